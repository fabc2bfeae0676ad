"""Shapelet initialisation from the training data: sliding k-means on the HIP kernels (ops.shapelet_kmeans_step / _update).

The reference draws every shapelet from N(0, 1) (IGN/model/Shapelet.py:58).  Learning Time-series Shapelets -- the method the
'LTS' registry entry is named after -- starts from the k-means centroids of the training segments instead: ``kmeans_init_`` does
that for every length group of an SBM / LTS / InterpGN model.  The distance of shapelet (k, c) reads channel c only, so each
(group, channel) clusters its own windows; nothing of the (B, Tw, K, C, L) broadcast is formed.
"""
import torch

from ign_hip import ops
from models.InterpGN import InterpGN
from models.Shapelet import ShapeBottleneckModel

_TENSOR_BATCH = 256       # rows per batch when `batches` is one (n, T, C) tensor


def _bottleneck(model):
    if isinstance(model, InterpGN):
        model = model.sbm
    if not isinstance(model, ShapeBottleneckModel):
        raise TypeError(f"kmeans_init_: expected an SBM, LTS or InterpGN model, got {type(model).__name__}")
    return model


def _collect(batches, max_batches, device):
    """The first `max_batches` batches as float32 (B, T, C) tensors on `device`.  A loader may draw from the global RNG when it
    is iterated (shuffling, worker seeds): the CPU stream is put back afterwards."""
    if torch.is_tensor(batches):
        if batches.dim() != 3:
            raise ValueError(f"kmeans_init_: a tensor of batches must be (n, T, C), got {tuple(batches.shape)}")
        batches = [(batches[i:i + _TENSOR_BATCH],) for i in range(0, batches.shape[0], _TENSOR_BATCH)]
    state = torch.get_rng_state()
    out = []
    try:
        for item in batches:
            if len(out) >= max_batches:
                break
            x = item[0] if isinstance(item, (tuple, list)) else item
            out.append(x.detach().to(device=device, dtype=torch.float32))
    finally:
        torch.set_rng_state(state)
    if not out:
        raise ValueError("kmeans_init_: no batches")
    return out


def draw_seed_windows(total, K, C, generator):
    """-> (K, C) int64 tensor: per channel K DISTINCT flat (sample, window) indices in [0, total), drawn on the host from
    `generator`.  Duplicates would give exact ties, hence empty clusters, from the first step."""
    if total < K:
        raise ValueError(f"kmeans_init_: {K} shapelets per channel need {K} distinct windows, the data has {total}")
    out = torch.empty(K, C, dtype=torch.int64)
    for c in range(C):
        seen = []
        while len(seen) < K:
            for v in torch.randint(total, (2 * K,), generator=generator).tolist():
                if v not in seen:
                    seen.append(v)
                    if len(seen) == K:
                        break
        out[:, c] = torch.tensor(seen)
    return out


def _seed_group(shp, xns, offsets, picks):
    """Copy the picked windows into shp.weights: picks (K, C) flat indices sample * Tw + window over the concatenated batches."""
    K, C, L = shp.weights.shape
    T = xns[0].shape[2]
    Tw = (T - L) // shp.stride + 1
    sample, window = picks // Tw, picks % Tw
    pos = torch.arange(L)
    for xn, lo in zip(xns, offsets):
        here = (sample >= lo) & (sample < lo + xn.shape[0])
        if not here.any():
            continue
        k, c = (i.to(xn.device) for i in here.nonzero(as_tuple=True))
        b = (sample[here] - lo).to(xn.device)
        t = (window[here] * shp.stride).to(xn.device).unsqueeze(1) + pos.to(xn.device)         # (n, L) sample positions
        shp.weights.data[k, c] = xn[b.unsqueeze(1), c.unsqueeze(1), t]


def kmeans_init_(model, batches, iters=10, max_batches=8, seed=0):
    """Replace the shapelets of `model` (SBM, LTS or InterpGN) in place by k-means centroids of the training windows.

    batches: a loader yielding (x[B,T,C], y, mask) or an (n, T, C) tensor; the first `max_batches` batches are used.
    Seeds: per (length group, channel) K distinct (sample, window) pairs from a private host generator seeded with `seed` (the
    global RNG streams are not touched).  Each of the `iters` Lloyd iterations streams the batches through ops.instance_norm and
    one accumulating ops.shapelet_kmeans_step per group, then updates each group once.  Ties go to the lowest k and an empty
    cluster keeps its centroid (constant or padded stretches can hold bit-equal windows; that is not an error).  LTS thresholds
    and every other parameter are left alone.  A cluster of one window ends as an exact copy of it: the x == w case
    Shapelet.tie_exact exists for.
    -> {"groups": [{"length", "stride", "inertia": [per iteration, summed over the channels in float64], "counts": (K,C) int32
    CPU tensor of the last iteration, "empty": clusters without a window in the last iteration}, ...], "iters", "batches",
    "windows": [windows per channel and group]}."""
    sbm = _bottleneck(model)
    iters, max_batches = int(iters), int(max_batches)
    if iters < 1 or max_batches < 1:
        raise ValueError(f"kmeans_init_: iters={iters} and max_batches={max_batches} must be at least 1")
    device = sbm.shapelets[0].weights.device
    xs = _collect(batches, max_batches, device)
    offsets, n = [], 0
    for x in xs:
        offsets.append(n)
        n += x.shape[0]
    gen = torch.Generator().manual_seed(int(seed))
    report = {"groups": [], "iters": iters, "batches": len(xs), "windows": []}
    with torch.no_grad():
        xns = [ops.instance_norm(x)[0] for x in xs]
        T = xns[0].shape[2]
        for shp in sbm.shapelets:
            K, C, L = shp.weights.shape
            Tw = (T - L) // shp.stride + 1
            _seed_group(shp, xns, offsets, draw_seed_windows(n * Tw, K, C, gen))
            report["groups"].append({"length": L, "stride": shp.stride, "inertia": [], "counts": None, "empty": 0})
            report["windows"].append(n * Tw)
        del xns
        for _ in range(iters):
            stats = [None] * len(sbm.shapelets)
            for x in xs:
                xn = ops.instance_norm(x)[0]
                for g, shp in enumerate(sbm.shapelets):
                    st = stats[g] or (None, None, None)
                    stats[g] = ops.shapelet_kmeans_step(xn, shp.weights, shp.stride, *st)
            for g, shp in enumerate(sbm.shapelets):
                sums, counts, inertia = stats[g]
                ops.shapelet_kmeans_update(shp.weights.data, sums, counts)
                rec = report["groups"][g]
                rec["inertia"].append(float(inertia.double().sum().item()))
                rec["counts"] = counts
        for rec in report["groups"]:
            rec["counts"] = rec["counts"].cpu()
            rec["empty"] = int((rec["counts"] == 0).sum().item())
    return report
