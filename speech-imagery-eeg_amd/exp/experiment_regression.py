"""Regression experiment harness -- drop-in for IGN/exp/experiment_regression.py.

Same surface: ``Experiment(args)`` with ``model_dict`` (no EEGCNN), ``train()``, ``validation()`` (-> val loss),
``test(save_csv, result_dir)`` (-> ``(crps, None, df)``), ``checkpoint_dir`` (same scheme), ``model`` and ``loss_fn`` (the
torch ``CRPSLoss`` holding the train split's ``bin_edges``).  The real-valued target is binned into the train split's 10
equal-width bins and the models are trained as 10-"class" classifiers under the CRPS of the softmax CDF (:59-76).

Everything else is the classification harness (subclassed, not copied): flat-buffer Adam, device prefetch, DDP, early
stopping -- on the validation loss here (:195) -- and the ``--hipgraph`` step.  On the GPU the loss tail is one HIP launch
per loss call (ops.crps_loss / ops.ign_crps_loss); the torch ``CRPSLoss`` is the CPU path.

Repairs of fork defects: the target stays float32 and is compared in float64 with the edges (R1, the reference
truncates it with ``.long()``); every batch is padded to the dataset's max_seq_len and subsampled with one fixed stride (R2,
data_provider); ``DNN`` receives ``configs`` only (R3).  InterpGN gets the ``--num_shapelet`` lists here (the 6 x K bank),
as the reference's regression twin does (:126-138).
"""
import os
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn as nn

from data_provider.data_factory import data_provider
from exp.experiment_classification import Experiment as ClassificationExperiment
from exp.experiment_classification import get_dnn_model
from ign_hip import ops as ign_ops
from models.InterpGN import InterpGN
from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
from utils.tools import gini_coefficient

SHAPELET_LENGTHS = [0.05, 0.1, 0.2, 0.3, 0.5, 0.8]


class CRPSLoss(nn.Module):
    """IGN/exp/experiment_regression.py:59-76: mean_b sum_j (cumsum(softmax(pred))_bj - [bin_edges_j >= target_b])^2, with
    the target kept real-valued (R1).  The torch statement, for CPU runs; the GPU runs ops.crps_loss."""

    def __init__(self, bin_edges):
        super().__init__()
        self.register_buffer("bin_edges", torch.as_tensor(bin_edges, dtype=torch.float64))

    def forward(self, pred, target):
        cdf_pred = torch.cumsum(torch.softmax(pred.float(), dim=1), dim=1)
        cdf_true = (self.bin_edges.unsqueeze(0) >= target.reshape(-1, 1).double()).float()
        return torch.mean(torch.sum((cdf_pred - cdf_true) ** 2, dim=1))


class Experiment(ClassificationExperiment):
    model_dict = {
        'InterpGN': InterpGN,
        'SBM': ShapeBottleneckModel,
        'LTS': DistThresholdSBM,
        'DNN': get_dnn_model,
    }

    def __init__(self, args):
        super().__init__(args)
        self.bin_edges = np.asarray(self.train_data.bin_edges, dtype=np.float64)
        self.loss_fn = CRPSLoss(torch.from_numpy(self.bin_edges)).to(self.device)
        self.edges = self.loss_fn.bin_edges                  # (N,) float64 on the device: the kernels' bin edges

    def _load_data(self):
        # val is the TEST split, as in the reference (:86-88, D6); both receive the train split's bin edges
        self.train_data, self.train_loader = data_provider(self.args, flag="train")
        edges = self.train_data.bin_edges
        self.test_data, self.test_loader = data_provider(self.args, flag="test", bin_edges=edges)
        self.val_data, self.val_loader = data_provider(self.args, flag="val", bin_edges=edges)

    def _build_model(self):
        a = self.args
        if a.model not in self.model_dict:
            raise ValueError(f"model {a.model!r} not in {list(self.model_dict)}")
        if a.model == 'DNN':                                 # R3: get_dnn_model takes configs only
            return self.model_dict['DNN'](a)
        return self.model_dict[a.model](configs=a, num_shapelet=[a.num_shapelet] * len(SHAPELET_LENGTHS),
                                        shapelet_len=SHAPELET_LENGTHS)

    def _to_device(self, batch_x, label, padding_mask):
        batch_x = batch_x.float().to(self.device, non_blocking=True)
        label = label.float().reshape(-1).to(self.device, non_blocking=True)       # real-valued targets (R1)
        padding_mask = padding_mask.float().to(self.device, non_blocking=True)
        return batch_x, label, padding_mask

    def _crps(self, logits, target):
        if logits.is_cuda:
            return ign_ops.crps_loss(logits, target, self.edges)
        return self.loss_fn(logits, target)

    def _train_loss(self, logits, info, label, beta, amp):
        """CRPS(out) [+ info.loss.mean()] [+ beta*CRPS(sbm)] (:155-169); InterpGN's whole tail is one launch on the GPU."""
        a = self.args
        if a.model == 'InterpGN' and logits.is_cuda:
            reg = info.loss
            fused_reg = reg.dtype == torch.float32 and reg.numel() == 1
            loss = ign_ops.ign_crps_loss(info.shapelet_preds, info.dnn_preds, label, self.edges, beta,
                                         reg=reg if fused_reg else None)[0]
            return loss if fused_reg else loss + reg.float().mean()
        loss = self._crps(logits, label)
        if a.model != 'DNN':
            loss = loss + info.loss.mean()
        if a.model == 'InterpGN':
            loss = loss + beta * self._crps(info.shapelet_preds, label)
        return loss

    def _eval_loss(self, logits, info, label):
        """Validation / test loss of one batch: CRPS(out) + info.loss.mean() (:209-222, :262-268)."""
        loss = self._crps(logits, label)
        if self.args.model != 'DNN':
            loss = loss + info.loss.mean()
        return loss.float()

    def _val_metrics(self):
        return self.validation(), None

    def validation(self):
        """-> mean validation loss over the series (each batch weighted by its size, so the value does not depend on
        --batch_size)."""
        if len(self.val_loader) == 0:
            return float('inf')
        amp = self.args.amp and self.device.type == 'cuda'
        total, n = [], 0
        self.model.eval()
        with torch.no_grad():
            for batch_x, label, padding_mask in self.val_loader:
                batch_x, label, padding_mask = self._to_device(batch_x, label, padding_mask)
                with torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=amp):
                    logits, info = self._forward(batch_x, padding_mask)
                    total.append(self._eval_loss(logits, info, label) * label.shape[0])
                n += label.shape[0]
        self.model.train()
        return torch.stack(total).sum().item() / n

    def test(self, save_csv=True, result_dir=None):
        """-> (test CRPS, None, df) (:233-353; ``gating_value`` is applied here only).  df: x, pred, target and, for the
        shapelet models, predicate, w, shapelets, eta, sbm_pred."""
        if result_dir is not None:
            os.makedirs(result_dir, exist_ok=True)
        if len(self.test_loader.dataset) == 0:
            return float('inf'), None, None
        a = self.args
        amp = a.amp and self.device.type == 'cuda'

        @dataclass
        class Buffer:
            x_data: list = field(default_factory=list)
            trues: list = field(default_factory=list)
            preds: list = field(default_factory=list)
            shapelet_preds: list = field(default_factory=list)
            p: list = field(default_factory=list)
            eta: list = field(default_factory=list)
            loss: list = field(default_factory=list)

        buf = Buffer()       # accumulators stay on the device; one host copy per field after the loop
        self.model.eval()
        with torch.no_grad():
            for batch_x, label, padding_mask in self.test_loader:
                if batch_x.size(0) == 0:
                    continue
                batch_x, label, padding_mask = self._to_device(batch_x, label, padding_mask)
                with torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=amp):
                    logits, info = self._forward(batch_x, padding_mask, gating_value=a.gating_value, test=True)
                    buf.loss.append(self._eval_loss(logits, info, label) * label.shape[0])
                buf.x_data.append(batch_x)
                buf.trues.append(label)
                buf.preds.append(logits.float())
                if a.model != 'DNN':
                    buf.p.append(info.p.float())
                    buf.shapelet_preds.append(info.shapelet_preds.float())
                    if a.model == 'InterpGN':
                        buf.eta.append(info.eta.float())
        if not buf.trues:
            return float('inf'), None, None
        host = lambda parts: torch.cat(parts).cpu()
        trues = host(buf.trues)
        test_loss = torch.stack(buf.loss).sum().item() / len(trues)
        if self.rank == 0:
            print(f"Test: n={len(trues)} CRPS loss={test_loss:.6f}")
        df = {'x': host(buf.x_data).float().numpy(), 'pred': host(buf.preds).numpy(), 'target': trues.float().numpy()}
        row = {k: getattr(a, k) for k in self.SUMMARY_ARGS if hasattr(a, k)}
        row['test_loss'] = test_loss
        row['epoch_stop'] = self.epoch_stop
        if a.model != 'DNN':
            sbm = self.model.sbm if a.model == 'InterpGN' else self.model
            w = sbm.output_layer.weight.detach().float().cpu()
            eta = host(buf.eta) if a.model == 'InterpGN' else None
            df.update(predicate=host(buf.p).numpy(), w=w.numpy(), shapelets=sbm.get_shapelets(),
                      eta=None if eta is None else eta.numpy(),
                      sbm_pred=host(buf.shapelet_preds).numpy() if a.model == 'InterpGN' else None)
            row['eta_mean'] = float(eta.mean()) if eta is not None else None
            row['eta_std'] = float(eta.std()) if eta is not None else None
            for name, thr in (('10', 1), ('5', 0.5), ('1', 0.1)):       # the column names of :305-332
                big = (w.abs() > thr).float()
                row[f'w_sum_{name}'] = float(big.sum())
                row[f'w_mean_{name}'] = float(big.mean())
            row['w_max'] = float(w.abs().max())
            row['w_gini_clip'] = float(gini_coefficient(np.clip(w.numpy(), 0, None)))
            row['w_gini_abs'] = float(gini_coefficient(np.abs(w.numpy())))
            src = self._shapelet_sources_for_test()
            if src is not None:                 # --shapelet_project: which training window every shapelet is a copy of
                df.update(shapelet_source=src["source"].numpy(), shapelet_source_start=src["start"].numpy(),
                          shapelet_source_d=src["d_before"].numpy())
        row.update(self._project_summary())
        if save_csv and result_dir is not None and self.rank == 0:
            self._write_row(row, result_dir)
        return test_loss, None, df

    def _write_row(self, row, result_dir):
        import csv
        from datetime import datetime
        a = self.args
        stamp = datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
        path = os.path.join(result_dir, f"{a.dataset}-{a.seed}-{a.model}-{a.num_shapelet}-{a.lambda_div}-{a.lambda_reg}-{stamp}.csv")
        with open(path, "w", newline="") as f:
            wr = csv.DictWriter(f, fieldnames=list(row))
            wr.writeheader()
            wr.writerow(row)
        print(f"Test summary saved at: {path}")
        return path
