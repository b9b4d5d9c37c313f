"""Generate the ReLU-SAE golden vectors (G19) by RUNNING the upstream reference (build container only).

Test infrastructure beside ``oracle/gen_golden.py`` (which it imports for its helpers and the reference import shim and
leaves unchanged).  The reference is read from its own location at generation time only; the outputs are data under
``tests/golden/``:

  g19_relu_forward_sparse   a ReLU SAE written by the reference's nn.dump (negative b_enc: tens of positives per row, one
                            all-zero input row with no positive at all), x, the reference's x_hats (one prefix) and x_hats
                            with three Matryoshka prefixes for every row, and its dense h_x / f_x for the first ROWS_DENSE
                            rows (the zero row among them; whole dense matrices would only make the file large)
  g19_relu_forward_dense    the same at random-init biases (about half of the latents fire: more than the engine's default
                            row capacity of 512 in some rows)
  g19_inference_relu_plain  the reference's framework/inference.worker_fn on a ReLU SAE over a small protocol-2.1 cache
  g19_inference_relu_labels the same with labels.bin and ignore_labels=[2]

    python tools/gen_relu_golden.py
"""

import importlib
import json
import pathlib
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT))
import gen_golden as G  # noqa: E402

PREFIXES = (128, 512, 1024)
ROWS_DENSE = 8  # rows whose dense h_x / f_x are stored
ZERO_ROW = 5     # the all-zero input row of the sparse fixture


def make_relu_sae(ref, d, s, seed, l1=4e-4):
    torch.manual_seed(seed)
    cfg = ref.modeling.SparseAutoencoderConfig(
        d_model=d, d_sae=s, reinit_blend=0.0,
        activation=ref.modeling.Relu(sparsity=ref.modeling.L1Sparsity(coeff=l1)))
    sae = ref.modeling.SparseAutoencoder(cfg)
    with torch.no_grad():
        sae.b_enc.copy_(0.05 * torch.randn(s))
        sae.b_dec.copy_(0.1 * torch.randn(d))
        sae.W_enc.add_(0.02 * torch.randn(d, s))
    return sae


def forward_fixture(ref, tag, sparse):
    d, s, n = 16, 1024, 70  # n not a multiple of the encoder's 32-row tile
    sae = make_relu_sae(ref, d, s, seed=190 + sparse)
    x = G.lowrank_data(n, d, seed=192 + sparse)
    if sparse:
        x[ZERO_ROW] = 0.0  # h = b_enc < 0 everywhere: a row without positives
        with torch.no_grad():
            h0 = x @ sae.W_enc
            sae.b_enc.copy_(-torch.quantile(h0.flatten(), 0.97) + 0.02 * torch.randn(s))
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="g19_"))
    try:
        ref.modeling.dump(tmp / "sae.pt", sae)
        ckpt = (tmp / "sae.pt").read_bytes()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with torch.no_grad():
        out = sae(x)
        x_hats_p = sae.decode(out.f_x, prefixes=torch.tensor(PREFIXES, dtype=torch.int64))
    nnz = (out.f_x > 0).sum(dim=1)
    print(f"{tag}: positives per row min {int(nnz.min())} median {int(nnz.median())} max {int(nnz.max())}")
    if sparse:
        assert int(nnz[ZERO_ROW]) == 0 and int(nnz.max()) < 512
    else:
        assert int(nnz.max()) > 512, "the dense fixture must overflow the default row capacity"
    # the parameters travel inside the checkpoint only (the reference's own nn.dump bytes)
    G.npz(f"g19_relu_forward_{tag}", ckpt=np.frombuffer(ckpt, dtype=np.uint8), x=x, h_x=out.h_x[:ROWS_DENSE],
          f_x=out.f_x[:ROWS_DENSE], x_hats=out.x_hats, x_hats_p=x_hats_p, prefixes=np.array(PREFIXES, dtype=np.int64),
          zero_row=ZERO_ROW if sparse else -1)


def inference_fixture(ref, tag, with_labels):
    """framework/inference.worker_fn of the reference on a ReLU SAE (as G14 does for TopK, oracle/gen_golden.py)."""
    import scipy.sparse

    from saev_amd.data import shards as my_shards

    ordered = importlib.import_module("saev.data.ordered")
    ref.data.OrderedConfig, ref.data.OrderedDataLoader = ordered.Config, ordered.DataLoader
    inf = importlib.import_module("saev.framework.inference")
    rshards = importlib.import_module("saev.data.shards")

    d, s, n_ex, n_tok, layers = 32, 256, 13, 6, (5, 11)
    rows = G.lowrank_data(n_ex * len(layers) * (n_tok + 1), d, seed=195 + with_labels)
    acts = rows.reshape(n_ex, len(layers), n_tok + 1, d).numpy()
    labels = None
    if with_labels:
        labels = np.random.default_rng(19).integers(0, 4, (n_ex, n_tok)).astype(np.uint8)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="g19_"))
    try:
        shards_dir = my_shards.write_shards(tmp, acts, layers=layers, cls_token=True,
                                            max_tokens_per_shard=4 * (n_tok + 1) * len(layers), labels=labels)
        md = rshards.Metadata.load(shards_dir)
        sae = make_relu_sae(ref, d, s, seed=197)
        # the first bias draw with no near-tie at the ReLU cut (|h| >= 2e-5 in fp64 on every token of the layer), so that the
        # CSR structure is the same under any fp32 summation order
        x_layer = torch.from_numpy(acts[:, layers.index(11), 1:, :].reshape(-1, d)).double()
        for bias_seed in range(198, 298):
            b_enc = -0.6 + 0.05 * torch.randn(s, generator=torch.Generator().manual_seed(bias_seed))
            if (x_layer @ sae.W_enc.detach().double() + b_enc.double()).abs().min() >= 2e-5:
                break
        else:
            raise RuntimeError("no bias draw without a near-tie")
        with torch.no_grad():
            sae.b_enc.copy_(b_enc)
            sae.b_dec.copy_(rows.mean(dim=0))
        run = G.ref_disk_new(tmp, shards_dir)
        ref.modeling.dump(run / "checkpoint" / "sae.pt", sae)
        cfg = inf.Config(run=run, data=ordered.Config(shards=shards_dir, layer=11, batch_size=4 * n_tok + 1),
                         n_dists=5, ignore_labels=[2] if with_labels else [], device="cpu")
        inf.worker_fn(cfg)
        out = run / "inference" / md.hash
        csr = scipy.sparse.load_npz(out / "token_acts.npz")
        metrics = json.loads((out / "metrics.json").read_text())
        print(f"inference {tag}: {csr.nnz} codes over {csr.shape[0]} tokens")
        G.npz(f"g19_inference_relu_{tag}", acts=acts, labels=labels if labels is not None else np.zeros((0, 0), np.uint8),
              layers=np.array(layers), n_dists=5, batch_size=4 * n_tok + 1,
              max_tokens_per_shard=4 * (n_tok + 1) * len(layers),
              ignore_labels=np.array([2] if with_labels else [], dtype=np.int64),
              ckpt=np.frombuffer((run / "checkpoint" / "sae.pt").read_bytes(), dtype=np.uint8),
              csr_data=csr.data, csr_indices=csr.indices, csr_indptr=csr.indptr, csr_shape=np.array(csr.shape),
              mean_values=torch.load(out / "mean_values.pt"), sparsity=torch.load(out / "sparsity.pt"),
              distributions=torch.load(out / "distributions.pt"),
              metrics_keys=np.array(list(metrics.keys())), metrics_vals=np.array([float(v) for v in metrics.values()]),
              **G.params_of(sae))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ref = G._refshim.install()
    forward_fixture(ref, "sparse", True)
    forward_fixture(ref, "dense", False)
    inference_fixture(ref, "plain", False)
    inference_fixture(ref, "labels", True)


if __name__ == "__main__":
    main()
