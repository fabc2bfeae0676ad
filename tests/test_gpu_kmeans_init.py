"""Shapelet initialisation by sliding k-means on the GPU (csrc/ign_shapelet_kmeans.hip, utils/shapelet_init.py).

The reference has no such feature, so the yardstick is `lloyd_ref` below: one Lloyd step restated in float64 torch (unfold,
mean squared difference, first-index argmin, one-hot einsum)."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import make_cfg, parity

pytestmark = pytest.mark.gpu

# (B, C, T, K, L, stride): the smallest shapes that reach a distinct path each
BASE = (6, 3, 80, 4, 9, 1)
SHAPES = [BASE,                         # baseline
          (4, 5, 300, 5, 33, 1),        # odd L, several windows per lane
          (3, 2, 1100, 5, 100, 1),      # row longer than 1024 samples (two passes over the row)
          (3, 3, 3100, 3, 310, 8),      # the reference's stride rule
          (2, 122, 200, 5, 20, 1),      # CHISCO's channel count
          (6, 3, 80, 7, 9, 1),          # more than one K tile (5 + 2)
          (6, 3, 80, 17, 9, 1)]         # ... (5 + 5 + 5 + 2; three accumulate tiles)
NEAR_TIE, MAX_LEFT_OUT = 1e-4, 0.01


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _ops():
    import speech_imagery_eeg_amd  # noqa: F401
    from ign_hip import ops
    return ops


def lloyd_ref(xn, w, stride, assign=None):
    """One Lloyd step in float64 on the CPU.  xn (B,C,T), w (K,C,L) -> dict: d (B,C,Tw,K), the first-index argmin `a`, and for the
    assignment used (`assign`, default `a`) sums (K,C,L), counts (K,C), inertia (C) and the updated centroids (an empty cluster
    keeps its row of w)."""
    xn, w = xn.double().cpu(), w.double().cpu()
    K, C, L = w.shape
    win = xn.unfold(2, L, stride)                                               # (B,C,Tw,L)
    d = ((win.unsqueeze(3) - w.permute(1, 0, 2)[None, :, None]) ** 2).mean(-1)  # (B,C,Tw,K)
    a = d.argmin(-1)
    use = a if assign is None else assign.long().cpu()
    onehot = F.one_hot(use, K).double()
    sums = torch.einsum("bctk,bctl->kcl", onehot, win)
    counts = onehot.sum((0, 2)).t().contiguous()                                # (K,C)
    inertia = d.gather(-1, use.unsqueeze(-1)).sum((0, 2, 3))
    new = torch.where(counts.unsqueeze(-1) > 0, sums / counts.clamp(min=1).unsqueeze(-1), w)
    return dict(d=d, a=a, sums=sums, counts=counts.long(), inertia=inertia, centroids=new)


def _data(shape, seed=0):
    """Instance-normalised batch on the GPU and K DISTINCT data windows per channel as the centroids."""
    ops = _ops()
    B, C, T, K, L, stride = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, generator=g).cumsum(1) * 0.3 + torch.randn(B, T, C, generator=g)      # drift + noise
    xn = ops.instance_norm(x.to(_dev()))[0]
    Tw = (T - L) // stride + 1
    w = torch.empty(K, C, L)
    xc = xn.cpu()
    for c in range(C):
        for k, flat in enumerate(torch.randperm(B * Tw, generator=g)[:K].tolist()):
            b, t = divmod(flat, Tw)
            w[k, c] = xc[b, c, t * stride:t * stride + L]
    return xn, w.to(xn.device)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(xn, w, float64 reference of one step), computed once per shape and shared, never modified"""
    xn, w = _data(shape)
    return xn, w, lloyd_ref(xn, w, shape[5])


def check_step(label, xn, w, stride, ref=None):
    """Run one step on the GPU and compare it with float64 as the issue sets: assignments exact outside the near-tie set (two
    smallest float64 distances within 1e-4 of the larger; at most 1 % of the windows), counts = histogram of the kernel's own
    assignment, centroids and inertia at the project's 1e-4 against float64 on the kernel's own assignment."""
    ops = _ops()
    ref = ref or lloyd_ref(xn, w, stride)
    K = w.shape[0]
    sums, counts, inertia, assign = ops.shapelet_kmeans_step(xn, w, stride, return_assign=True)
    a = assign.cpu().long()
    assert a.shape == ref["a"].shape and int(a.min()) >= 0 and int(a.max()) < K
    if K > 1:
        two = ref["d"].topk(2, dim=-1, largest=False).values
        near = (two[..., 1] - two[..., 0]) <= NEAR_TIE * two[..., 1]
    else:
        near = torch.zeros_like(a, dtype=torch.bool)
    share = near.double().mean().item()
    wrong = int(((a != ref["a"]) & ~near).sum())
    print(f"{label}: near-tie share {share:.5f}, mismatches outside it {wrong}, inside it {int(((a != ref['a']) & near).sum())}")
    assert share <= MAX_LEFT_OUT, f"{label}: {share:.4f} of the windows are near-ties"
    assert wrong == 0, f"{label}: {wrong} assignments differ from float64 outside the near-tie set"
    hist = F.one_hot(a, K).sum((0, 2)).t()
    assert torch.equal(counts.cpu().long(), hist), f"{label}: counts are not the histogram of assign"
    own = lloyd_ref(xn, w, stride, assign=a)
    new = ops.shapelet_kmeans_update(w.clone(), sums, counts)
    parity(f"{label}.centroids", new, own["centroids"], kind="elem", ref_is="float64 Lloyd step on the kernel's assignment")
    parity(f"{label}.inertia", inertia, own["inertia"], kind="scale", ref_is="float64 Lloyd step on the kernel's assignment")
    return sums, counts, inertia, assign, new


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_against_float64(shape):
    xn, w, ref = _case(shape)
    check_step("step", xn, w, shape[5], ref)


def test_far_centroid_stays_empty_and_is_kept_bit_for_bit():
    ops = _ops()
    xn, w, _ = _case(BASE)
    w = w.clone()
    w[2] = 100.0
    sums, counts, _ = ops.shapelet_kmeans_step(xn, w)
    assert int(counts[2].abs().sum()) == 0 and int(counts.sum()) == BASE[0] * BASE[1] * (BASE[2] - BASE[4] + 1)
    new = ops.shapelet_kmeans_update(w.clone(), sums, counts)
    assert torch.equal(new[2], w[2])
    for k in (0, 1, 3):
        assert not torch.equal(new[k], w[k])


def test_duplicate_centroid_loses_every_tie_to_the_lower_index():
    ops = _ops()
    xn, w, _ = _case(BASE)
    w = w.clone()
    w[1] = w[0]
    _, counts, _, assign = ops.shapelet_kmeans_step(xn, w, return_assign=True)
    assert int(counts[1].sum()) == 0 and int((assign == 1).sum()) == 0 and int(counts[0].sum()) > 0


def test_same_call_twice_is_bitwise_equal():
    ops = _ops()
    for shape in (SHAPES[1], SHAPES[3]):
        xn, w, _ = _case(shape)
        r1 = ops.shapelet_kmeans_step(xn, w, shape[5], return_assign=True)
        r2 = ops.shapelet_kmeans_step(xn, w, shape[5], return_assign=True)
        assert all(torch.equal(a, b) for a, b in zip(r1, r2))
        assert torch.equal(ops.shapelet_kmeans_update(w.clone(), r1[0], r1[1]), ops.shapelet_kmeans_update(w.clone(), r2[0], r2[1]))


def test_two_accumulated_halves_equal_the_whole_batch():
    ops = _ops()
    shape = (40, 3, 80, 4, 9, 1)                        # 10 batch slices; the halves 5 each
    xn, w = _data(shape, seed=3)
    whole = ops.shapelet_kmeans_step(xn, w)
    acc = ops.shapelet_kmeans_step(xn[:20], w)
    out = ops.shapelet_kmeans_step(xn[20:], w, 1, *acc)
    assert all(o is a for o, a in zip(out, acc))        # accumulated in place
    assert torch.equal(whole[1], acc[1])
    parity("halves.centroids", ops.shapelet_kmeans_update(w.clone(), acc[0], acc[1]),
           ops.shapelet_kmeans_update(w.clone(), whole[0], whole[1]), kind="elem", ref_is="one call on the whole batch")
    parity("halves.inertia", acc[2], whole[2], kind="scale", ref_is="one call on the whole batch")


def test_teacher_forced_trajectory():
    """6 float64 Lloyd iterations; at each, the kernel is fed the float64 centroids and compared as a single step."""
    shape = SHAPES[1]
    xn, w, _ = _case(shape)
    w64 = w.double().cpu()
    last = None
    for it in range(6):
        ref = lloyd_ref(xn, w64, shape[5])
        check_step(f"iter{it}", xn, w64.float().to(xn.device), shape[5])
        total = float(ref["inertia"].sum())
        assert last is None or total <= last * (1 + 1e-12)
        last, w64 = total, ref["centroids"]


def _batches(n, T, C, nb, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, T, C, generator=g).cumsum(1) * 0.3 + torch.randn(n, T, C, generator=g)
    return x, [(xb, torch.zeros(xb.shape[0], 1), torch.ones(xb.shape[0], T)) for xb in x.chunk(nb)]


@pytest.mark.parametrize("lts", [False, True], ids=["SBM", "LTS"])
def test_kmeans_init_free_running(lts):
    dev = _dev()
    import speech_imagery_eeg_amd  # noqa: F401
    from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
    from oracle import ign_oracle as O
    from utils.shapelet_init import kmeans_init_
    cfg = make_cfg(enc_in=5, seq_len=120, num_class=3)
    torch.manual_seed(0)
    m = (DistThresholdSBM if lts else ShapeBottleneckModel)(cfg, [3, 3, 3], [0.1, 0.3, 0.6]).to(dev)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, batches = _batches(16, 120, 5, 2, seed=7)              # two loader-style batches of 8
    cpu_state, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    rep = kmeans_init_(m, batches, iters=6, max_batches=8, seed=0)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
    after = m.state_dict()
    for k, v in before.items():
        if k.endswith(".weights"):
            assert not torch.equal(after[k], v), k
        else:
            assert torch.equal(after[k], v), k           # thresholds, class head: untouched
    assert rep["iters"] == 6 and rep["batches"] == 2 and len(rep["groups"]) == 3
    for g, s in zip(rep["groups"], m.shapelets):
        h = g["inertia"]
        print(f"L={g['length']}: inertia {h}, empty {g['empty']}")
        assert len(h) == 6 and all(b <= a * (1 + 1e-4) for a, b in zip(h, h[1:])) and h[-1] < h[0]
        assert g["length"] == s.length and g["counts"].shape == (3, 5)
        assert int(g["counts"].sum()) == 5 * 16 * (120 - s.length + 1) and g["empty"] == int((g["counts"] == 0).sum())

    # the initialised model against the oracle loaded with the same state dict; a centroid can be an exact copy of a window,
    # which is what the exact sign(0) = 0 backward passes are for
    m.set_tie_exact(True)
    ref = O.OracleSBM(cfg, [3, 3, 3], [0.1, 0.3, 0.6], lts=lts)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    y = torch.arange(16) % 3
    o_r, i_r = ref(x)
    (F.cross_entropy(o_r, y) + i_r.loss.mean()).backward()
    o, i = m(x.to(dev))
    (F.cross_entropy(o, y.to(dev)) + i.loss.mean()).backward()
    parity("init.out", o, o_r, kind="elem", ref_is="CPU oracle fp32")
    parity("init.p", i.p, i_r.p, kind="elem", ref_is="CPU oracle fp32")
    ref_params = dict(ref.named_parameters())
    for n, p in m.named_parameters():
        parity(f"init.grad.{n}", p.grad, ref_params[n].grad, kind="scale", floor=1e-6, ref_is="CPU oracle fp32")


def _run_driver(tmp, name, extra, capsys, monkeypatch):
    import speech_imagery_eeg_amd  # noqa: F401
    import run
    os.makedirs(tmp / name)
    monkeypatch.chdir(tmp / name)
    run.main(["--data", "SYNTH", "--synthetic", "32,4,64,3", "--model", "SBM", "--train_epochs", "1", "--batch_size", "8",
              "--seed", "0", "--amp", "--log_interval", "1", "--num_shapelet", "3"] + extra)
    out = capsys.readouterr().out
    ckpt = [os.path.join(d, f) for d, _, fs in os.walk(tmp / name / "checkpoints") for f in fs if f == "checkpoint.pth"]
    assert len(ckpt) == 1, out[-2000:]
    return out, torch.load(ckpt[0], map_location="cpu", weights_only=True)


def test_driver_kmeans_flag_and_unchanged_default(tmp_path, capsys, monkeypatch):
    _dev()
    out, sd = _run_driver(tmp_path, "kmeans", ["--shapelet_init", "kmeans", "--shapelet_init_iters", "3",
                                               "--shapelet_init_batches", "2"], capsys, monkeypatch)
    lines = re.findall(r"^shapelet_init kmeans: length (\d+) inertia (\S+) -> (\S+) \(3 iterations, 2 batches\) empty clusters (\d+)$",
                       out, flags=re.M)
    assert [int(l[0]) for l in lines] == [4, 7, 13, 20, 32, 52], out[-3000:]            # the SBM's six length groups at T = 64
    assert all(float(l[2]) <= float(l[1]) * (1 + 1e-4) for l in lines)
    assert re.search(r"^Epoch 1/1 \| Train Loss ", out, flags=re.M) and "accuracy:" in out
    # the default: nothing runs, and two runs are the same run, loss lines and trained weights
    out1, sd1 = _run_driver(tmp_path, "normal1", [], capsys, monkeypatch)
    out2, sd2 = _run_driver(tmp_path, "normal2", ["--shapelet_init", "normal"], capsys, monkeypatch)
    assert "shapelet_init kmeans" not in out1 + out2
    pick = lambda o: [re.sub(r" \| Time Rem .*", "", l) for l in o.splitlines() if l.startswith(("Epoch ", "accuracy:"))]
    assert pick(out1) == pick(out2) and len(pick(out1)) == 2
    assert sd1.keys() == sd2.keys() and all(torch.equal(sd1[k], sd2[k]) for k in sd1)
    assert any(not torch.equal(sd[k], sd1[k]) for k in sd if k.endswith(".weights"))
