"""Shapelet projection: snap every learned shapelet to the nearest real training window and keep where it came from.

A trained shapelet is a free (K, C, L) parameter -- a curve no electrode ever produced.  ``project_`` replaces every shapelet of
an SBM / LTS / InterpGN model by the training window nearest to it under the model's own distance and reports, per shapelet,
the sample and the window it now is a bit-exact copy of ("samples 312-411 of trial 57 on electrode 14").  The sliding distances,
their per-sample minimum and its location are the model's own forward (``ShapeBottleneckModel.shapelet_features``); the
reduction over the training set and the gather of the winner are ops.shapelet_project_bank (csrc/ign_shapelet_project.hip).
"""
import json

import torch

from ign_hip import _lib, ops
from models.InterpGN import InterpGN
from models.Shapelet import ShapeBottleneckModel

_TENSOR_BATCH = 256       # rows per batch when `batches` is one (n, T, C) tensor


def _bottleneck(model):
    if isinstance(model, InterpGN):
        model = model.sbm
    if not isinstance(model, ShapeBottleneckModel):
        raise TypeError(f"project_: expected an SBM, LTS or InterpGN model, got {type(model).__name__}")
    return model


def _stream(batches, device):
    """Yield (x (B,T,C) float32 on `device`, keep-mask or None) for every batch, in the order given."""
    if torch.is_tensor(batches):
        if batches.dim() != 3:
            raise ValueError(f"project_: a tensor of batches must be (n, T, C), got {tuple(batches.shape)}")
        batches = [(batches[i:i + _TENSOR_BATCH],) for i in range(0, batches.shape[0], _TENSOR_BATCH)]
    for item in batches:
        x, mask = item, None
        if isinstance(item, (tuple, list)):
            x = item[0]
            mask = item[2] if len(item) > 2 else None
        if x.shape[0] == 0:
            continue
        yield x.detach().to(device=device, dtype=torch.float32), mask


def project_(model, batches, lengths_from_mask=None):
    """Replace the shapelets of `model` (SBM, LTS or InterpGN) in place by their nearest training windows.

    batches: a loader yielding (x[B,T,C], y, mask) or an (n, T, C) tensor, streamed once IN THE ORDER GIVEN: the sample ordinals
    of the report count that stream (data_provider.data_factory.ordered_loader makes them data set indices).  Under
    torch.no_grad() and outside autocast; a loader may draw from the global RNG when it is iterated: the CPU stream is put back.
    Per batch: sbm.shapelet_features, then one ops.shapelet_project_bank call.  "Nearest" is nearest under the model's own
    distance (the forward produced it); ties go to the lowest (sample, window).  lengths_from_mask: None = model.mask_padding;
    when on and the batch carries a keep-mask, every sample is matched over its own length, so neither padding windows nor
    samples shorter than a shapelet take part; off: the reference's behaviour, the padding takes part.
    Afterwards each group's `weights` hold the winners -- copied into the existing storage (FlatParamBucket views and captured
    graphs keep pointing at it); a shapelet without any candidate keeps its value.  LTS thresholds, heads and optimiser state
    are not touched.
    -> {"groups": [{"length", "stride", "source": (K,C,2) int32 CPU tensor of (sample ordinal, window), "start": (K,C) int32 =
    window * stride, "d_before": (K,C) distance to the winner before the copy, "kept": shapelets without a candidate (source
    -1, start -1, d_before +inf)}, ...], "source" (F,2), "start" (F,), "d_before" (F,), "length" (F,): the same in feature-column
    order g*K*C + k*C + c, "samples", "batches"}."""
    sbm = _bottleneck(model)
    use_lengths = sbm.mask_padding if lengths_from_mask is None else bool(lengths_from_mask)
    device = sbm.shapelets[0].weights.device
    shapes = [tuple(s.weights.shape) for s in sbm.shapelets]
    strides = [int(s.stride) for s in sbm.shapelets]
    states, n, nb = None, 0, 0
    rng = torch.get_rng_state()
    try:
        with torch.no_grad(), torch.autocast(device_type=device.type, enabled=False):
            for x, mask in _stream(batches, device):
                if use_lengths and mask is not None:
                    lengths = mask.to(device).sum(1).to(torch.int32)
                    xn = ops.instance_norm_len(x, lengths)
                    _, d, t = sbm.shapelet_features(x, None, lengths)
                else:
                    xn, _ = ops.instance_norm(x)
                    _, d, t = sbm.shapelet_features(x, xn, None)
                states = ops.shapelet_project_bank(xn, d, t, shapes, strides, n, states)
                n += x.shape[0]
                nb += 1
    finally:
        torch.set_rng_state(rng)
    if states is None:
        raise ValueError("project_: no batches")
    report = {"groups": [], "samples": n, "batches": nb}
    with torch.no_grad():
        for shp, (best_d, src, cand) in zip(sbm.shapelets, states):
            found = (src[..., 0] >= 0).unsqueeze(-1)
            shp.weights.data.copy_(torch.where(found, cand, shp.weights.data))
            source = src.cpu()
            window = source[..., 1]
            report["groups"].append({
                "length": shp.length, "stride": int(shp.stride), "source": source,
                "start": torch.where(window >= 0, window * int(shp.stride), window), "d_before": best_d.cpu(),
                "kept": int((source[..., 0] < 0).sum().item())})
        _lib.PARAM_GENERATION[0] += 1        # parameter values changed behind autograd's back (see _lib.PARAM_GENERATION)
    groups = report["groups"]
    report["source"] = torch.cat([g["source"].reshape(-1, 2) for g in groups])
    report["start"] = torch.cat([g["start"].reshape(-1) for g in groups])
    report["d_before"] = torch.cat([g["d_before"].reshape(-1) for g in groups])
    report["length"] = torch.cat([torch.full((g["source"].shape[0] * g["source"].shape[1],), g["length"], dtype=torch.int32)
                                  for g in groups])
    return report


def sources_table(report):
    """The report of project_ as one JSON-able record per feature column: column, group, k, c, index (sample ordinal; the data
    set index after an ordered pass), window, start, length, d_before -- index / window / start -1 and d_before null for a
    shapelet that was kept."""
    rows = []
    for g, rec in enumerate(report["groups"]):
        K, C = rec["source"].shape[:2]
        for k in range(K):
            for c in range(C):
                idx, win = (int(v) for v in rec["source"][k, c])
                rows.append({"column": len(rows), "group": g, "k": k, "c": c, "index": idx, "window": win,
                             "start": int(rec["start"][k, c]), "length": int(rec["length"]),
                             "d_before": float(rec["d_before"][k, c]) if idx >= 0 else None})
    return rows


def save_sources(path, report):
    """Write the sidecar of a projected checkpoint (shapelet_sources.json) -> path."""
    with open(path, "w") as f:
        json.dump({"version": 1, "samples": int(report["samples"]), "columns": sources_table(report)}, f, indent=1)
    return path


def load_sources(path):
    """-> {"source" (F,2) int32, "start" (F,) int32, "length" (F,) int32, "d_before" (F,) float32 (+inf where kept), "columns":
    the records as written} from a sidecar written by save_sources."""
    with open(path) as f:
        cols = json.load(f)["columns"]
    return {"source": torch.tensor([[r["index"], r["window"]] for r in cols], dtype=torch.int32).reshape(-1, 2),
            "start": torch.tensor([r["start"] for r in cols], dtype=torch.int32),
            "length": torch.tensor([r["length"] for r in cols], dtype=torch.int32),
            "d_before": torch.tensor([float("inf") if r["d_before"] is None else r["d_before"] for r in cols], dtype=torch.float32),
            "columns": cols}
