"""Golden fixtures for the regression task (--task_name regression), from the reference.

Run (CPU only, under a minute):   python tests/golden/make_golden_regression.py

Imports the reference exactly as make_golden.py does (its shims are reused by import, `_import_data_factory` binds the
reference's vendored Monash parser) and writes arrays only:
  crps_loss.npz                  the reference CRPSLoss value and its autograd gradient: real-valued targets, N in {2, 10, 39},
                                 targets below the first edge, on an edge and above the last finite edge
  monash_contract.npz            the reference Monashloader over the generated `@targetLabel` files tests/golden/ts/Reg*.ts:
                                 equal length (TRAIN + TEST with the train edges), ragged, missing values
  train_step_ign_regression.npz  InterpGN(FCN) with 6 groups x 2 shapelets, 10 bins: forward, CRPS(out) + reg + beta*CRPS(sbm),
                                 gradients, and three Adam steps (lr 5e-3) on float targets
The reference truncates targets with `.long()` before its CRPS (repair R1); the fixtures feed the float targets
straight into its CRPSLoss, which is the intended behaviour.  Weights are rounded to fp16-representable values and stored as
float16 (exact); large tensors' gradients / final weights are stored as (norm, fixed sample) to keep each file under 1 MiB.
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_many_class as MC  # noqa: E402

SHAPELET_LENGTHS = [0.05, 0.1, 0.2, 0.3, 0.5, 0.8]


def _crps_cls():
    MG.import_reference()
    MG._import_data_factory()
    with contextlib.redirect_stdout(io.StringIO()):
        return importlib.import_module("exp.experiment_regression").CRPSLoss


def monash_edges(y, nbins):
    """the rule of IGN/data_factory/data_loader.py:798-810 (restated here only to build inputs; the loader case checks it)"""
    e = np.linspace(float(np.min(y)), float(np.max(y)), nbins + 1)
    e[0], e[-1] = -np.inf, np.inf
    return e[1:]


def case_crps_loss(R=None):
    CRPSLoss = _crps_cls()
    out = {}
    g = torch.Generator().manual_seed(2024)
    for N in (2, 10, 39):
        lo = -1.5
        hi = lo + 0.25 * N                               # bin width 0.25: every edge is exact in float32
        edges = monash_edges(np.array([lo, hi]), N)
        B = 37
        y = (torch.rand(B, generator=g) * (hi - lo) + lo).float()
        y[0] = lo - 3.0                                  # below the first edge: H = 1 everywhere
        y[1] = float(edges[N // 2 - 1]) if N > 2 else float(edges[0])      # exactly on an edge: counts as >=
        y[2] = hi + 2.0                                  # above the last finite edge: only the +inf bin is 1
        y[3] = float(edges[-2]) if N > 2 else float(edges[0])              # on the last finite edge
        z = (torch.randn(B, N, generator=g) * 2.0).requires_grad_(True)
        loss = CRPSLoss(torch.from_numpy(edges))(z, y)
        loss.backward()
        out.update({f"n{N}_logits": MG.npy(z), f"n{N}_target": MG.npy(y), f"n{N}_edges": edges,
                    f"n{N}_loss": np.float64(loss.item()), f"n{N}_grad": MG.npy(z.grad)})
    MG.save("crps_loss", **out)


def _write_reg_ts(tsdir):
    """Small Monash-format files (generated text, committed as data): `@targetLabel true` and a float target after the last ':'"""
    os.makedirs(tsdir, exist_ok=True)
    rng = np.random.RandomState(11)

    def series(n):
        return ",".join(repr(round(float(v), 4)) for v in rng.randn(n) * 2 + 0.5)

    head = ("@problemName {name}\n@timeStamps false\n@missing {miss}\n@univariate false\n@dimensions 2\n@equalLength {eq}\n{sl}"
            "@targetLabel true\n@data\n")
    files = {}
    for split, n in (("TRAIN", 9), ("TEST", 5)):
        t = rng.randn(n) * 4 + 10
        if split == "TEST":
            t[0], t[1] = -50.0, 80.0                     # outside the train range
        body = "".join(":".join(series(24) for _ in range(2)) + ":" + repr(round(float(t[i]), 5)) + "\n" for i in range(n))
        files[f"RegEq_{split}.ts"] = head.format(name="RegEq", miss="false", eq="true", sl="@seriesLength 24\n") + body
    lens = [14, 24, 19, 7, 24, 11]
    t = rng.randn(len(lens)) * 3
    body = "".join(":".join(series(L) for _ in range(2)) + ":" + repr(round(float(t[i]), 5)) + "\n" for i, L in enumerate(lens))
    files["RegRagged_TRAIN.ts"] = head.format(name="RegRagged", miss="false", eq="false", sl="") + body
    rows = []
    t = rng.rand(5) * 100
    for i in range(5):
        dims = []
        for d in range(2):
            vals = [repr(round(float(v), 4)) for v in rng.randn(16)]
            for j in rng.choice(16, size=3, replace=False):
                vals[j] = "?"
            if i == 3 and d == 0:
                vals[0] = vals[-1] = "?"
            dims.append(",".join(vals))
        rows.append(":".join(dims) + ":" + repr(round(float(t[i]), 5)) + "\n")
    files["RegMissing_TRAIN.ts"] = head.format(name="RegMissing", miss="true", eq="true", sl="@seriesLength 16\n") + "".join(rows)
    for name, text in files.items():
        with open(os.path.join(tsdir, name), "w", encoding="utf-8") as f:
            f.write(text)
    return sorted(files)


def case_monash_contract(R=None):
    import warnings
    warnings.simplefilter("ignore")
    D = MG._import_data_factory()
    tsdir = os.path.join(HERE, "ts")
    _write_reg_ts(tsdir)
    out = {}
    sink = io.StringIO()
    train_edges = None
    for fname in ("RegEq_TRAIN.ts", "RegEq_TEST.ts", "RegRagged_TRAIN.ts", "RegMissing_TRAIN.ts"):
        stem = fname[:-3]
        edges = train_edges if fname == "RegEq_TEST.ts" else None
        with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
            ds = D["data_loader"].Monashloader(tsdir, bin_edges=edges, file_list=[fname])
        if fname == "RegEq_TRAIN.ts":
            train_edges = ds.bin_edges
        out[f"{stem}_edges"] = np.asarray(ds.bin_edges, dtype=np.float64)
        out[f"{stem}_feature"] = ds.feature_df.values.astype(np.float64)
        out[f"{stem}_index"] = np.asarray(ds.feature_df.index, dtype=np.int64)
        out[f"{stem}_target"] = ds.labels_df.values.astype(np.float64)
        out[f"{stem}_maxlen"] = np.int64(ds.max_seq_len)
    MG.save("monash_contract", **out)


def case_train_step_ign_regression(R):
    CRPSLoss = _crps_cls()
    N, B = 10, 8
    c = MG.cfg(num_class=N, c_out=N)
    torch.manual_seed(0)
    m = R["InterpGN"].InterpGN(c, num_shapelet=[2] * 6, shapelet_len=SHAPELET_LENGTHS)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    sd0 = MC.sd_half(m, "sd0.")
    g = torch.Generator().manual_seed(313)
    xs = torch.randn(3, B, 100, 6, generator=g)
    ys = (torch.randn(3, B, generator=g) * 2.0 + 1.0).float()
    edges = monash_edges(ys.numpy(), N)
    crps = CRPSLoss(torch.from_numpy(edges))
    beta = 1.0
    opt = torch.optim.Adam(m.parameters(), lr=5e-3)
    losses, extra = [], {}
    m.train()
    for i in range(3):
        out, info = m(xs[i], torch.ones(B, 100), None, None)
        loss = crps(out, ys[i]) + info.loss.mean() + beta * crps(info.shapelet_preds, ys[i])
        loss.backward()
        if i == 0:
            extra.update(out0=MG.npy(out), sbm0=MG.npy(info.shapelet_preds), dnn0=MG.npy(info.dnn_preds), eta0=MG.npy(info.eta),
                         reg0=np.float64(info.loss.mean().item()), crps_out0=np.float64(crps(out, ys[i]).item()),
                         crps_sbm0=np.float64(crps(info.shapelet_preds, ys[i]).item()), **MG.grads_compact(m, "grad0."))
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    MG.save("train_step_ign_regression", xs=MG.npy(xs), ys=MG.npy(ys), edges=edges, beta=np.float64(beta),
            losses=np.array(losses, dtype=np.float64), **sd0, **MC.sd_compact(m, "sd3."), **extra)


CASES = {
    "crps_loss": case_crps_loss,
    "monash_contract": case_monash_contract,
    "train_step_ign_regression": case_train_step_ign_regression,
}

if __name__ == "__main__":
    R = MG.import_reference()
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name](R)
