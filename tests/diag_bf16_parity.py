"""Diagnostic (not a test): the noise floor of the float64 attention model of tests/test_gpu_bf16_parity.py, and the assembly of
profiles/bf16_parity.json.  Needs no GPU.

--noise-floor: per attention shape the model (_attn_model) is run twice, the second time with every intermediate in front of a bf16
  rounding point moved by a relative 2^-23 (random sign, fixed seed: _fp32_noise); prints the distance between the two runs for out,
  dq, dk, dv (_rel and _rms_rel) and the model's distance to the unrounded float64 attention.  The largest noise figures are
  ATTN_NOISE / ATTN_NOISE_RMS of the test module, the bounds ATTN_FACTOR times that; every quantity whose distance to the unrounded
  result is not 10x above its bound is listed.
--misplaced: the model with one rounding point moved (edits of its source text), its distance to the model per shape and quantity:
  what the bounds can and cannot tell apart.
--cases FILE (repeatable): a JSON object merged into the output -- the record a GPU run of the test module wrote
  (IGN_BF16_PARITY_OUT=cases.json), a record of planted-error runs.
Usage: python tests/diag_bf16_parity.py --noise-floor --misplaced [--cases cases.json] --out profiles/bf16_parity.json"""
import argparse
import inspect
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_gpu_bf16_parity as T  # noqa: E402

QUANT = ("out", "dq", "dk", "dv")
METRICS = (("rel", T._rel), ("rms_rel", T._rms_rel))


def _shape_name(sh):
    return "B={} L={} S={} H={} E={}".format(*sh)


def noise_floor(seed):
    rows, worst = {}, {m: 0.0 for m, _ in METRICS}
    for sh in T._ATTN_SHAPES:
        q, k, v, go = T._attn_inputs(*sh)
        scale = 1.0 / math.sqrt(sh[-1])
        clean = T._attn_model(q, k, v, go, scale)
        noisy = T._attn_model(q, k, v, go, scale, pre=T._fp32_noise(seed))
        exact = T._attn_exact(q, k, v, go, scale)
        row = {}
        for what in QUANT:
            row[what] = {}
            for m, f in METRICS:
                row[what][m] = dict(noise=f(noisy[what], clean[what]), model_vs_unrounded=f(clean[what], exact[what]))
                worst[m] = max(worst[m], row[what][m]["noise"])
        rows[_shape_name(sh)] = row
        print(_shape_name(sh) + ": " + "  ".join(f"{w} noise {r['rel']['noise']:.2e} (rms {r['rms_rel']['noise']:.2e}) / unrounded "
                                                 f"{r['rel']['model_vs_unrounded']:.2e} (rms {r['rms_rel']['model_vs_unrounded']:.2e})"
                                                 for w, r in row.items()), flush=True)
    res = dict(seed=seed, perturbation="relative 2^-23, random sign, on every fp32 intermediate in front of a bf16 rounding point",
               factor=T.ATTN_FACTOR, per_shape=rows,
               constants_in_the_test=dict(ATTN_NOISE=T.ATTN_NOISE, ATTN_NOISE_RMS=T.ATTN_NOISE_RMS, ATTN_TOL=T.ATTN_TOL,
                                          ATTN_TOL_RMS=T.ATTN_TOL_RMS))
    for m, _ in METRICS:
        tol = T.ATTN_FACTOR * worst[m]
        close = [f"{s}: {w}" for s, row in rows.items() for w, r in row.items() if not r[m]["model_vs_unrounded"] >= 10 * tol]
        res[m] = dict(noise=worst[m], bound=tol, less_than_10x_from_the_unrounded_result=close)
        print(f"{m}: noise {worst[m]:.3e} x {T.ATTN_FACTOR} = bound {tol:.3e}; {len(close)} of {len(rows) * len(QUANT)} quantities are "
              f"less than 10x the bound from the unrounded result")
    return res


_MISPLACED = {
    "P rounded after normalisation": [('einsum("bhls,bshd->bhld", r(p), vr[:, s0:s0 + 32])', 'einsum("bhls,bshd->bhld", p, vr[:, s0:s0 + 32])'),
                                      ("out = (O / l[..., None])",
                                       "out = torch.einsum('bhls,bshd->bhld', r(torch.exp2(S2 - (m + torch.log2(l))[..., None])), vr)")],
    "row sum l from the rounded p": [("l = l * alpha + p.sum(-1)", "l = l * alpha + r(p).sum(-1)")],
    "delta from the rounded dO": [("(gf.double() * out)", "(gr * out)")],
    "dO not rounded": [("gr = r(qf), r(kf), r(vf), r(gf)", "gr = r(qf), r(kf), r(vf), gf.double()")],
    "dS not rounded": [("r(dS)", "dS"), ("r(dSb)", "dSb")],
    "dK / dV score with the factor on q": [('einsum("blhe,bshe->bhls", qr, ks)', 'einsum("blhe,bshe->bhls", qs, kr)')],
}


def misplaced():
    src = inspect.getsource(T._attn_model)
    res = {}
    for name, edits in _MISPLACED.items():
        s = src
        for old, new in edits:
            assert old in s, (name, old)
            s = s.replace(old, new)
        ns = dict(vars(T))
        exec(s, ns)
        res[name] = {}
        for sh in T._ATTN_SHAPES:
            q, k, v, go = T._attn_inputs(*sh)
            scale = 1.0 / math.sqrt(sh[-1])
            clean, moved = T._attn_model(q, k, v, go, scale), ns["_attn_model"](q, k, v, go, scale)
            row = {w: {m: f(moved[w], clean[w]) for m, f in METRICS} for w in QUANT}
            res[name][_shape_name(sh)] = row
            seen = [w for w in QUANT if row[w]["rms_rel"] > T.ATTN_TOL_RMS or row[w]["rel"] > T.ATTN_TOL]
            print(f"{name} | {_shape_name(sh)}: " + "  ".join(f"{w} {row[w]['rel']:.2e} (rms {row[w]['rms_rel']:.2e})" for w in QUANT)
                  + f"  beyond a bound: {seen}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise-floor", action="store_true")
    ap.add_argument("--misplaced", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cases", action="append", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {}
    if a.noise_floor:
        out["attention_noise_floor"] = noise_floor(a.seed)
    if a.misplaced:
        out["attention_model_with_one_rounding_point_moved"] = misplaced()
    for path in a.cases:
        with open(path) as f:
            out.update(json.load(f))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
