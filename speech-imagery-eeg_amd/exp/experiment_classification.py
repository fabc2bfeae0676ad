"""Classification experiment harness -- drop-in for IGN/exp/experiment_classification.py.

Same surface: ``Experiment(args)`` with ``model_dict``, ``train()``, ``validation()``, ``test(save_csv, result_dir)``,
``checkpoint_dir``, ``model``; same loss composition (:319-329), accumulation / clipping / Adam / clamp order
(:331-341), early stopping on ``-val_accuracy`` and best-checkpoint reload (:360-376), checkpoint path scheme
(:140-152).  What is new underneath: the models run the HIP shapelet kernels, and under ``torch.distributed``
(one process per GPU) gradients are averaged with one flat RCCL all-reduce per step (ign_hip.ddp) instead of
``nn.DataParallel``.

Deliberate repairs of fork defects: dataset parameters are taken from the dataset object for
UEA too (D5); ``EEGCNN`` receives (B,C,T) and no mask (D9); ``np.Inf`` is not used (D12).  Reproduced as-is: IGN is
built WITHOUT the ``--num_shapelet`` lists (D4), ``--amp`` switches bf16 autocast OFF (D3).
"""
import contextlib
import os
import sys
import time
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from data_provider.data_factory import data_provider
from data_provider.device_prefetch import DevicePrefetcher
from ign_hip import ddp as ign_ddp
from ign_hip import ops as ign_ops
from ign_hip.ddp import FlatAdam, FlatParamBucket
from models.FullyConvNet import FullyConvNetwork
from models.InterpGN import InterpGN, dnn_dict
from models.Shapelet import DistThresholdSBM, ShapeBottleneckModel
from utils.shapelet_util import ClassificationResult
from utils.tools import EarlyStopping, convert_to_hms, gini_coefficient, per_class_metrics  # noqa: F401


def compute_beta(epoch, max_epoch, schedule='cosine'):
    """Weight of the auxiliary SBM cross-entropy (IGN/exp/experiment_classification.py:19-26)."""
    if schedule == 'cosine':
        return 1 / 2 * (1 + np.cos(np.pi * epoch / max_epoch))
    if schedule == 'linear':
        return 1 - epoch / max_epoch
    return 1


def compute_shapelet_score(shapelet_distances, cls_weights, y_pred, y_true):
    """:29-34 -- mean class-weighted distance score over correctly classified samples."""
    score = shapelet_distances @ F.relu(cls_weights.T) / shapelet_distances.shape[-1]
    ok = y_pred == y_true
    return score[ok].gather(-1, y_true[ok].unsqueeze(1)).mean().item()


def get_dnn_model(configs):
    return dnn_dict[configs.dnn_type](configs)


def get_eegcnn_model(configs):
    from models.eegcnn import EEGCNNTransformer
    return EEGCNNTransformer(configs)


def accuracy_score(pred, true):
    pred, true = np.asarray(pred), np.asarray(true)
    return float((pred == true).mean()) if len(true) else 0.0


def _raw_training_batches(exp):
    """The raw TRAINING trials of an experiment in data set order, un-sharded and un-augmented, as (X (B,C,T), y, gid): on the GPU the
    loader's own raw batches, moved to the device; else host arrays from the data set."""
    from data_provider.data_factory import ordered_loader
    if getattr(exp.train_loader, 'eeg_chain', None) is not None:                  # raw items: the loader's own batches
        batches = ordered_loader(exp.train_loader)
        return DevicePrefetcher(batches, exp.device) if exp.device.type == 'cuda' else batches
    return exp.train_data.raw_batches(exp.args.batch_size)


class Experiment(object):
    model_dict = {
        'InterpGN': InterpGN,
        'SBM': ShapeBottleneckModel,
        'LTS': DistThresholdSBM,
        'DNN': get_dnn_model,
        'EEGCNN': get_eegcnn_model,
    }
    class_weight, label_smoothing = None, 0.0       # the training criterion's options (_resolve_loss_options)
    _optim_active, _ema = False, False              # --weight_decay / --lr_schedule / --ema (_resolve_optim_options)

    def __init__(self, args):
        self.args = args
        self.distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.rank = dist.get_rank() if self.distributed else 0
        self.world = dist.get_world_size() if self.distributed else 1
        if torch.cuda.is_available():
            self.device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)) if self.distributed else 0)
        else:
            self.device = torch.device('cpu')
        self._resolve_optim_options()   # --weight_decay / --lr_schedule / --ema: what is refused raises before anything is built

        self._load_data()
        self._report_eeg_artifact()     # --eeg_artifact ...,report: one pass over the raw training trials, before the model is built
        self._get_params_from_data()
        self._resolve_loss_options()
        self._resolve_train_transforms()
        # host -> device double buffering (and, for raw CHISCO shards, the on-GPU standardise + transpose)
        self.train_loader, self.val_loader, self.test_loader = (self._prefetch(l) for l in
                                                                (self.train_loader, self.val_loader, self.test_loader))

        self.model = self._build_model().to(self.device)
        self._init_shapelets()          # --shapelet_init kmeans, on rank 0: before the flat bucket, whose broadcast carries it
        # On the GPU the step uses the flat path of bench.py: gradients are views into one buffer (a single RCCL all-reduce
        # under torch.distributed) and Adam is one ign_adam_step launch over the flat parameter buffer.
        self.bucket = None
        if self.distributed or self.device.type == 'cuda':
            self.bucket = FlatParamBucket(self.model, self.world)
            self.bucket.broadcast_state(0)
        if self.device.type == 'cuda' and self._optim_active:
            # AdamW / per-step schedule / EMA on the flat path; S = the run's optimizer steps (a step closes when the run-wide
            # batch count is a multiple of the accumulation)
            from utils.optim_rule import total_steps
            wd, spec, ema = self._optim_options
            self.optimizer = FlatAdam(self.bucket, lr=self.args.lr, weight_decay=wd, schedule=spec, ema=ema,
                                      total_steps=total_steps(self.args.train_epochs, len(self.train_loader),
                                                              self.args.gradient_accumulation_steps))
            if ema > 0.0 and self.args.pos_weight:
                # the average starts inside the constraint the clamp keeps the live weights in from the first step on: the model's
                # own clamp on the averaged copy (swapped in and out again; the live weights are not touched)
                self.optimizer.swap_ema()
                self.model.step()
                self.optimizer.swap_ema()
        elif self.device.type == 'cuda':
            self.optimizer = FlatAdam(self.bucket, lr=self.args.lr)
        else:
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=self.args.lr)
        # clipping and accumulation run on the flat buffer (ign_grad_norm_clip, ign_gather_flat_acc) when the optimizer is FlatAdam
        self._flat_step = isinstance(self.optimizer, ign_ddp.FlatAdam)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(self.optimizer, T_0=self.args.train_epochs)
        self.checkpoint_dir = "./checkpoints/{}/{}/dnn-{}_seed-{}_k-{}_div-{}_reg-{}_eps-{}_beta-{}_dfunc-{}_cls-{}".format(
            args.model, args.dataset, args.dnn_type, args.seed, args.num_shapelet, args.lambda_div, args.lambda_reg,
            args.epsilon, args.beta_schedule, args.distance_func, args.sbm_cls)
        if self.rank == 0:
            os.makedirs(self.checkpoint_dir, exist_ok=True)
            if getattr(self.train_data, 'chain', None) is not None:       # eeg_spatial.npz, eeg_iir.json, eeg_resample.json: what ran
                self.train_data.chain.save(self.checkpoint_dir)
        self.loss_fn = nn.CrossEntropyLoss()
        self.epoch_stop = 0
        print(f"Experiment: model={args.model} dnn={getattr(args, 'dnn_type', None)} device={self.device} "
              f"world={self.world} seq_len={args.seq_len} enc_in={args.enc_in} num_class={args.num_class} "
              f"train/val/test={len(self.train_data)}/{len(self.val_data)}/{len(self.test_data)}")

    def _init_shapelets(self):
        """--shapelet_init kmeans: the shapelets of an SBM / LTS / InterpGN model start as k-means centroids of the training
        windows (utils/shapelet_init.py) instead of N(0,1).  Rank 0 only; not under --test_only.  The default does nothing."""
        a = self.args
        how = getattr(a, 'shapelet_init', 'normal')
        if how == 'normal':
            return
        if how != 'kmeans':
            raise ValueError(f"shapelet_init must be normal|kmeans, got {how!r}")
        if getattr(a, 'mask_padding', False):
            raise ValueError("--shapelet_init kmeans with --mask_padding: k-means would cluster windows of the zero padding "
                             "(there is no length-aware k-means step); use --shapelet_init normal")
        if a.model not in ('SBM', 'LTS', 'InterpGN'):
            if self.rank == 0:
                print(f"--shapelet_init kmeans: model {a.model} has no shapelets, nothing to initialise")
            return
        if getattr(a, 'test_only', False) or self.rank != 0:
            return
        from utils.shapelet_init import kmeans_init_
        rep = kmeans_init_(self.model, self.train_loader, iters=getattr(a, 'shapelet_init_iters', 10),
                           max_batches=getattr(a, 'shapelet_init_batches', 8), seed=max(int(getattr(a, 'seed', 0)), 0))
        for g in rep["groups"]:
            print(f"shapelet_init kmeans: length {g['length']} inertia {g['inertia'][0]:.6g} -> {g['inertia'][-1]:.6g} "
                  f"({rep['iters']} iterations, {rep['batches']} batches) empty clusters {g['empty']}")

    def _resolve_loss_options(self):
        """--class_weight / --label_smoothing -> self.class_weight (None, or ONE float32 (num_class,) device tensor, allocated here
        and never re-created, so a captured --hipgraph step replays it) and self.label_smoothing.  `balanced` counts the labels
        of the FULL training set, before any rank sharding: every DDP rank holds the same vector.  The values are checked here,
        once, on the host (positive, finite, one per class); ops.ign_loss trusts them.  Only the TRAINING criterion changes:
        validation and test losses stay plain cross-entropy, so early stopping and every reported number stay comparable.
        Under DDP and --gradient_accumulation_steps each rank / micro-batch takes its OWN weighted mean (divided by the sum of
        the weights of its own labels); the gradients are then averaged / accumulated exactly as without weights -- what torch
        DDP does with a weighted criterion."""
        from utils.class_weight import check_loss_options, resolve_class_weight
        spec, self.label_smoothing = check_loss_options(self.args, self.args.num_class)
        w = resolve_class_weight(spec, self.train_data, self.args.num_class, notice=print if self.rank == 0 else None)
        self.class_weight = None if w is None else w.to(self.device)
        if w is not None and self.rank == 0:
            print(f"class weights ({self.args.class_weight if spec == 'balanced' else 'given'}): "
                  f"{[round(float(v), 4) for v in w]}")

    def _resolve_train_transforms(self):
        """--warp / --augment / --mix -> self._transforms, the chain that both training loops call once per step
        (utils/train_transforms.py); false when all three are off: the loops then do nothing extra.  What is refused (--mix with
        the regression task) raises here, for callers that build the namespace themselves."""
        from utils.train_transforms import TrainTransforms
        self._transforms = TrainTransforms.from_args(self.args, self.rank)

    def _resolve_optim_options(self):
        """--weight_decay / --lr_schedule / --ema -> self._optim_options (weight decay, LrSchedule, EMA decay) and self._optim_active
        (False when all three are neutral, also for a namespace without the flags: the optimizer is then constructed and stepped
        exactly as before).  utils.optim_rule.check_optim_options refuses what run.check_args refuses, for callers that build the
        namespace themselves; there is no CPU twin of the flat path."""
        from utils.optim_rule import check_optim_options
        self._optim_options = wd, spec, ema = check_optim_options(self.args, flat_path=self.device.type == 'cuda')
        self._optim_active = wd > 0.0 or spec.active or ema > 0.0
        self._ema = ema > 0.0
        if self._optim_active and self.rank == 0:
            print(f"optimizer: AdamW weight_decay={wd:g} lr_schedule={spec.kind}"
                  + (f",warmup={spec.warmup}" if spec.active else "") + (f",min={spec.min_lr:g}" if spec.kind == 'cosine' else "")
                  + f" ema={ema:g}")

    @contextlib.contextmanager
    def _averaged_weights(self):
        """--ema: inside the block the model holds the averaged weights (FlatAdam.swap_ema: one in-place exchange of the two flat
        buffers), after it the live ones again, bit for bit.  BatchNorm running statistics stay the live ones
        (torch.optim.swa_utils' default).  Without --ema the block runs as it stands."""
        if not self._ema:
            yield
            return
        self.optimizer.swap_ema()
        try:
            yield
        finally:
            self.optimizer.swap_ema()

    def _load_data(self):
        self.train_data, self.train_loader = data_provider(self.args, flag="train")
        self.val_data, self.val_loader = data_provider(self.args, flag="val")
        self.test_data, self.test_loader = data_provider(self.args, flag="test")
        self._fit_eeg_spatial()

    def _report_eeg_artifact(self):
        """--eeg_artifact ...,report: one ordered pass over the raw training trials before the model is built, through the stage's
        kernels; counts per electrode the trials judged flat, noisy, non-finite or unrepaired.  Every rank computes the same counts
        (no collective); rank 0 prints the table, and the counts go into eeg_artifact.json beside the checkpoint.  Without the key
        nothing runs."""
        stage = getattr(self.train_data, 'artifact', None)
        if stage is None or not stage.spec.report:
            return
        stage.report_pass(_raw_training_batches(self))
        if self.rank == 0:
            for line in stage.report_lines():
                print(line)

    def _fit_eeg_spatial(self):
        """--eeg_spatial align=euclid: one ordered, un-sharded, un-augmented pass over the raw TRAINING trials before the model is
        built (utils.eeg_spatial.fit_alignment: ops.eeg_spatial + ops.eeg_gram per batch on the device, float64 on the host), also
        under --test_only; every rank runs the same pass and ends with the same bits, without a collective.  The fitted matrices go
        to all three splits.  Without the flag, or without align=, nothing runs."""
        stage = getattr(self.train_data, 'spatial', None)
        if stage is None or stage.spec.align == 'none':
            return
        from utils.eeg_spatial import fit_alignment
        batches = _raw_training_batches(self)
        art = getattr(self.train_data, 'artifact', None)
        if art is not None:                            # --eeg_artifact: the alignment is fitted on the repaired rows
            fix = art.device_fn(self.device) if self.device.type == 'cuda' else (lambda x, gid: art.apply(np.asarray(x))[0])
            batches = ((fix(x, gid), y, gid) for x, y, gid in batches)
        W = fit_alignment(batches, stage.W0, stage.groups, stage.spec.rtol, notice=print if self.rank == 0 else None,
                          post=self.train_data.chain.alignment_post(self.device))     # --eeg_iir: the Gram of the filtered rows
        for d in (self.train_data, self.val_data, self.test_data):
            d.spatial.W, d.spatial.fitted = W, True
        if self.rank == 0:
            print(f"eeg_spatial: Euclidean alignment of {stage.groups} group(s) fitted on {len(self.train_data)} training trials")

    def _sync_buffers(self, src=0):
        """floating-point buffers (BatchNorm running mean / variance) of rank `src` -> every rank"""
        for buf in self.model.buffers():
            if buf.dtype.is_floating_point:
                dist.broadcast(buf.data, src=src)

    def _prefetch(self, loader):
        # raw CHISCO items carry their resolved --eeg_* chain; built here, after _fit_eeg_spatial: the transform reads the fitted matrices
        chain = getattr(loader, 'eeg_chain', None)
        if chain is None:
            return loader if self.device.type != 'cuda' else DevicePrefetcher(loader, self.device)
        return DevicePrefetcher(loader, self.device, transform=chain.device_transform(self.device))

    # ------------------------------------------------------------------------------------------------
    def _get_params_from_data(self):
        """seq_len / enc_in / num_class from the dataset object (intended behaviour of :166-249; the UEA attribute
        names are honoured as in IGN/exp/experiment_regression.py:90-96)."""
        d = self.train_data
        if hasattr(d, 'seq_len'):
            self.args.seq_len = int(d.seq_len)
        elif hasattr(d, 'max_seq_len'):
            self.args.seq_len = int(d.max_seq_len)
        else:
            self.args.seq_len = int(d[0][0].shape[0])
        if hasattr(d, 'enc_in'):
            self.args.enc_in = int(d.enc_in)
        elif hasattr(d, 'feature_df'):
            self.args.enc_in = int(d.feature_df.shape[1])
        else:
            self.args.enc_in = int(d[0][0].shape[1])
        if hasattr(d, 'num_classes'):
            self.args.num_class = int(d.num_classes)
        elif hasattr(d, 'class_names'):
            self.args.num_class = len(d.class_names)
        else:
            raise ValueError("dataset exposes neither num_classes nor class_names")
        self.args.pred_len = 0
        self.args.label_len = 0
        self.args.c_out = self.args.num_class
        self.args.original_fs = getattr(d, 'original_fs', 500)
        self.args.target_fs = getattr(d, 'target_fs', 256)

    def _build_model(self):
        a = self.args
        if a.model not in self.model_dict:
            raise ValueError(f"model {a.model!r} not in {list(self.model_dict)}")
        if a.model in ('SBM', 'LTS'):               # :264-270
            lens = [0.05, 0.1, 0.2, 0.3, 0.5, 0.8]
            model = self.model_dict[a.model](configs=a, num_shapelet=[a.num_shapelet] * len(lens), shapelet_len=lens)
        else:                                        # InterpGN gets NO shapelet lists (D4): 4 groups x 5
            model = self.model_dict[a.model](a)
        if getattr(a, 'multi_gpu', False) and not self.distributed:
            print("--multi_gpu: nn.DataParallel is replaced by one process per GPU; launch with "
                  "`python -m torch.distributed.run --nproc-per-node N run.py ...` (running single-GPU now)")
        return model

    def print_args(self):
        for k in sorted(vars(self.args)):
            print(f"  {k}: {getattr(self.args, k)}")

    # ------------------------------------------------------------------------------------------------
    def _forward(self, batch_x, padding_mask, gating_value=None, test=False):
        a = self.args
        if a.model == 'DNN':
            return self.model(batch_x, padding_mask, None, None), None
        if a.model == 'EEGCNN':
            return self.model(batch_x.permute(0, 2, 1))                   # (B,C,T) view, no mask (D9); the model transposes in HIP
        if test:
            return self.model(batch_x, padding_mask, None, None, gating_value=gating_value)
        return self.model(batch_x, padding_mask, None, None)

    def _to_device(self, batch_x, label, padding_mask):
        batch_x = batch_x.float().to(self.device, non_blocking=True)
        label = label.long().to(self.device, non_blocking=True)
        if label.dim() > 1:
            label = label.squeeze(-1)
        padding_mask = padding_mask.float().to(self.device, non_blocking=True)
        return batch_x, label, padding_mask

    def train_one_epoch(self, epoch, train_step=0):
        """The inner loop of train() -- IGN/exp/experiment_classification.py:313-343 -- over self.train_loader (host batches
        copied by the DevicePrefetcher): -> (detached per-step losses, running step count).  Validation is the caller's."""
        a = self.args
        amp = a.amp and self.device.type == 'cuda'
        self.model.train()
        losses = []
        if self._graph_eligible(amp):
            return self._train_one_epoch_graphed(epoch, train_step)
        for batch_x, label, padding_mask in self.train_loader:
            train_step += 1
            batch_x, label, padding_mask = self._to_device(batch_x, label, padding_mask)
            batch_x, soft = self._transforms(batch_x, label, padding_mask, train_step)
            with torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=amp):
                logits, info = self._forward(batch_x, padding_mask)
                loss = self._train_loss(logits, info, label, compute_beta(epoch, a.train_epochs, a.beta_schedule), amp, *soft)
            if a.gradient_accumulation_steps > 1:
                loss = loss / a.gradient_accumulation_steps
            ign_ops.backward(loss)                 # = loss.backward() (a cached unit root gradient on the GPU)
            micro = train_step % a.gradient_accumulation_steps
            if self._flat_step and a.gradient_accumulation_steps > 1:
                # the micro-batch gradients are summed in the flat buffer: the first micro-step of a cycle overwrites the slots,
                # the later ones add (one launch each); p.grad is None again for the next backward pass
                self.bucket.gather(accumulate=micro != 1)
                if micro:
                    self.bucket.zero_grad()
            if micro == 0:
                self._optimizer_step()
            losses.append(loss.detach())
        return losses, train_step

    def _optimizer_step(self):
        """The tail of an optimizer step, eager or captured (IGN/exp/experiment_classification.py:335-341): all-reduce, clipped Adam,
        clamp, the EMA launch under --ema, zero_grad."""
        a = self.args
        max_norm = a.gradient_clip if a.gradient_clip > 0 else None
        if self.bucket is not None:
            self.bucket.allreduce()
        if self._flat_step:
            self.optimizer.step(max_norm=max_norm)
        else:
            if max_norm is not None:
                nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=max_norm)
            self.optimizer.step()
        if a.pos_weight:
            self.model.step()
        if self._ema:
            self.optimizer.ema_update()           # after the clamp: an average of clamped values stays inside the constraint
        if self.bucket is not None:
            self.bucket.zero_grad()
        else:
            self.optimizer.zero_grad()

    def _train_loss(self, logits, info, label, beta, amp, label_b=None, lam=None):
        """The training loss of one step (IGN/exp/experiment_classification.py:319-329); `beta` weighs InterpGN's SBM term.
        Every cross-entropy of it takes the run's class weights and label smoothing (_resolve_loss_options), and under --mix the
        soft labels (label, label_b, lam) of self._transforms: the fused tail's soft-label entry point for InterpGN, utils.mix.mix_cross_entropy
        where the criterion is torch's."""
        a = self.args
        w, eps = self.class_weight, self.label_smoothing
        if lam is not None:
            if a.model == 'InterpGN' and logits.is_cuda and not amp:
                return ign_ops.ign_loss(info.shapelet_preds, info.dnn_preds, label, beta, reg=info.loss, class_weight=w,
                                        label_smoothing=eps, y_b=label_b, lam=lam)[0]
            from utils.mix import mix_cross_entropy
            loss = mix_cross_entropy(logits, label, label_b, lam, w, eps)
            if a.model != 'DNN':
                loss = loss + info.loss.mean()
            if a.model == 'InterpGN':
                loss = loss + beta * mix_cross_entropy(info.shapelet_preds, label, label_b, lam, w, eps)
            return loss
        if a.model == 'InterpGN' and logits.is_cuda and not amp:
            # CE(mixture) + info.loss.mean() + beta*CE(sbm) and both logit gradients in one launch (ops.ign_loss)
            # instead of ~40 softmax / nll / mean kernels between the forward and the backward pass
            return ign_ops.ign_loss(info.shapelet_preds, info.dnn_preds, label, beta, reg=info.loss, class_weight=w,
                                    label_smoothing=eps)[0]
        loss = F.cross_entropy(logits, label, weight=w, label_smoothing=eps)
        if a.model != 'DNN':
            loss = loss + info.loss.mean()
        if a.model == 'InterpGN':
            loss = loss + beta * F.cross_entropy(info.shapelet_preds, label, weight=w, label_smoothing=eps)
        return loss

    # -- `--hipgraph`: the same step as above, captured once per (beta, lr) and replayed per batch ---------------------------------
    def _graph_eligible(self, amp):
        a = self.args
        if getattr(a, 'mask_padding', False):
            if getattr(a, 'hipgraph', False) and not getattr(self, '_mask_graph_notice', False):
                self._mask_graph_notice = True
                print("--mask_padding: the length-aware shapelet expert is not captured; --hipgraph ignored, training eagerly")
            return False
        return (getattr(a, 'hipgraph', False) and self.device.type == 'cuda' and not amp and not self.distributed
                and a.model in ('InterpGN', 'SBM', 'LTS') and self._flat_step and not self._attention_dropout_active())

    def _attention_dropout_active(self):
        """Attention dropout draws a fresh seed per call on the host; a captured graph would replay one mask (ops.attention refuses
        to be captured with p > 0), so such a model trains eagerly."""
        from layers.SelfAttention_Family import FullAttention
        for m in self.model.modules():
            if isinstance(m, FullAttention) and m.dropout.p > 0:
                return True
            if isinstance(m, nn.MultiheadAttention) and m.dropout > 0:
                return True
        return False

    def _train_one_epoch_graphed(self, epoch, train_step):
        from ign_hip.graph import GraphedTrainStep
        a = self.args
        beta = float(compute_beta(epoch, a.train_epochs, a.beta_schedule)) if a.model == 'InterpGN' else 0.0
        # with --lr_schedule the learning rate is read on the device (hp_dev): it is no kernel argument and no part of the key
        lr = None if self.optimizer.schedule.active else float(self.optimizer.param_groups[0]['lr'])
        if not self.optimizer.capturable:          # the step count moves to the device so that a captured launch sequence stays valid
            self.optimizer.make_capturable()

        # Gradient accumulation over K micro-batches: at most TWO graphs per key.  "micro" = forward, loss / K, backward and an
        # ADDING gather (ign_gather_flat_acc); "close" = the same, then all-reduce, gradient norm, clipped Adam, clamp -- and one
        # fill of the flat buffer at its end, so that every micro-step of every cycle, the first included, adds into zeros and
        # needs no overwriting variant of its own (0 + g = g: the sums are those of the eager loop, which overwrites in the
        # first micro-step).  K = 1 captures only "close", with the overwriting gather and no fill: the step as it always was.
        # max_norm is a kernel argument, constant over a run; the coefficient stays on the device, so a replay clips by the norm
        # of ITS gradients.
        K = a.gradient_accumulation_steps

        def step_fn(batch_x, label, padding_mask, *soft, close=True):         # soft: (label_b, lam) under --mix, else nothing
            logits, info = self._forward(batch_x, padding_mask)
            loss = self._train_loss(logits, info, label, beta, False, *soft)
            if K > 1:
                loss = loss / K
            ign_ops.backward(loss)
            if K > 1:
                self.bucket.gather(accumulate=True)
                if not close:
                    return loss.detach()
            self._optimizer_step()
            if K > 1:
                self.bucket.clear()
            return loss.detach()

        def micro_fn(batch_x, label, padding_mask, *soft):
            return step_fn(batch_x, label, padding_mask, *soft, close=False)

        if K > 1 and not getattr(self, '_graph_acc_primed', False):
            self.bucket.clear()                    # every micro-step adds: the first cycle starts from zeros as well
            self._graph_acc_primed = True
        losses, graphed, key = [], getattr(self, '_graphed', None), (beta, lr, a.batch_size)
        for batch_x, label, padding_mask in self.train_loader:
            train_step += 1
            batch_x, label, padding_mask = self._to_device(batch_x, label, padding_mask)
            # outside the graph: its static inputs take this batch and, under --mix, label_b / lam
            batch_x, soft = self._transforms(batch_x, label, padding_mask, train_step)
            inputs = (batch_x, label, padding_mask, *soft)
            kind, fn = ('close', step_fn) if train_step % K == 0 else ('micro', micro_fn)
            if batch_x.shape[0] != a.batch_size:                  # ragged last batch: eager
                losses.append(fn(*inputs).clone())
                continue
            if graphed is None or graphed[0] != key:
                graphed = self._graphed = (key, {})
            if kind not in graphed[1]:
                # beta and (without --lr_schedule) lr are kernel ARGUMENTS: a new value needs a new capture.  This batch runs eagerly
                # (which also performs every first-call initialisation outside the capture); the capture that follows records the
                # launch sequence without executing it, so the parameter trajectory is exactly the eager one
                losses.append(fn(*inputs).clone())
                graphed[1][kind] = GraphedTrainStep(fn, inputs, warmup=0)
                continue
            losses.append(graphed[1][kind](*inputs).clone())
        return losses, train_step

    def train(self):
        a = self.args
        torch.set_float32_matmul_precision('medium')          # :297 (affects only torch's own GEMMs)
        early_stopping = EarlyStopping(patience=a.patience, verbose=self.rank == 0, delta=0)
        t_start = time.time()
        train_step = 0
        project_every, project_end = self._project_schedule()          # --shapelet_project; (0, False) by default
        for epoch in range(a.train_epochs):
            if len(self.train_loader) == 0:
                continue
            losses, train_step = self.train_one_epoch(epoch, train_step)
            if not losses:
                continue
            train_loss = torch.stack(losses).mean().item()      # one host sync per epoch (the reference syncs per step)
            if project_every and (epoch + 1) % project_every == 0:
                self._project_shapelets()       # before validation: early stopping and the checkpoint see the projected model
            if self.distributed:
                # BatchNorm running statistics are per rank (each rank saw its own shards); the model that is validated,
                # early-stopped on and checkpointed is rank 0's, so every rank evaluates THAT one ...
                self._sync_buffers(0)
            # --ema: validation, early stopping and checkpoint.pth see the averaged weights (every rank holds the same average of the
            # same flat parameters); the live ones are back before the next training pass
            with self._averaged_weights():
                val_loss, val_acc = self._val_metrics()
                if self.distributed:
                    # ... and the stopping decision is taken from one (val_loss, val_acc) pair: ranks that disagreed by one
                    # flipped argmax would leave the epoch loop at different times and dead-lock in the next all-reduce
                    t = torch.tensor([val_loss, 0.0 if val_acc is None else val_acc], dtype=torch.float64, device=self.device)
                    dist.broadcast(t, src=0)
                    val_loss, val_acc = float(t[0]), (None if val_acc is None else float(t[1]))
                remain = (time.time() - t_start) * (a.train_epochs - epoch) / (epoch + 1)
                if (epoch + 1) % a.log_interval == 0 and self.rank == 0:
                    acc = "" if val_acc is None else f" | Val Acc {val_acc:.4f}"
                    lr = ""
                    if self._optim_active and self.optimizer.schedule.active:       # the last update's, from the host rule
                        lr = f" | LR {self.optimizer.lr_at(train_step // a.gradient_accumulation_steps):.3g}"
                    print(f"Epoch {epoch + 1}/{a.train_epochs} | Train Loss {train_loss:.4f} | Val Loss {val_loss:.4f}{acc} | "
                          f"Time Rem {convert_to_hms(remain)}{lr}")
                if a.lr_decay:
                    self.scheduler.step()
                if epoch >= a.min_epochs:
                    score = val_loss if val_acc is None else -val_acc    # early stopping on -val_accuracy; no accuracy: val loss
                    if self.rank == 0:
                        early_stopping(score, self.model, self.checkpoint_dir)
                    else:                                       # same decision on every rank, only rank 0 writes
                        early_stopping.save_checkpoint = lambda *_: None
                        early_stopping(score, self.model, self.checkpoint_dir)
            self.epoch_stop = epoch
            if early_stopping.early_stop:
                if self.rank == 0:
                    print("Early stopping")
                break
            sys.stdout.flush()
        if self.distributed:
            dist.barrier()
        best = os.path.join(self.checkpoint_dir, 'checkpoint.pth')
        if os.path.exists(best):
            self.model.load_state_dict(torch.load(best, map_location=self.device, weights_only=True))
        if project_end:
            self._project_final(best)
        return self.model

    # -- `--shapelet_project`: snap the shapelets to real training windows (utils/shapelet_project.py) ---------------------------
    def _project_schedule(self):
        """--shapelet_project -> (N, at_end): project after every N-th epoch's training pass (0: never) / after the best
        checkpoint is reloaded.  none (the default, also for a namespace without the flag): (0, False)."""
        how = getattr(self.args, 'shapelet_project', 'none')
        if how is None or how == 'none':
            return 0, False
        if how == 'end':
            return 0, True
        try:
            n = int(how)
        except (TypeError, ValueError):
            n = 0
        if n < 1:
            raise ValueError(f"shapelet_project must be none|end|N with N >= 1, got {how!r}")
        return n, True

    def _project_shapelets(self):
        """One projection of the model's shapelets onto the training set (shared by the classification and regression harnesses,
        like _init_shapelets): an ordered, un-sharded, un-augmented pass over the training data (data_factory.ordered_loader), so
        the reported sample ordinals are data set indices and, under several ranks, every rank computes the same bit-exact
        shapelets -- no collective.  Adam moments, thresholds and heads are left alone.  -> the report of project_, also kept as
        self._shapelet_sources; None when nothing was done (flag off, --test_only, a model without shapelets)."""
        a = self.args
        if self._project_schedule() == (0, False) or getattr(a, 'test_only', False):
            return None
        if a.model not in ('SBM', 'LTS', 'InterpGN'):
            if self.rank == 0 and not getattr(self, '_project_notice', False):
                print(f"--shapelet_project: model {a.model} has no shapelets, nothing to project")
            self._project_notice = True
            return None
        from data_provider.data_factory import ordered_loader
        from utils.shapelet_project import project_
        rep = project_(self.model, ordered_loader(self.train_loader))
        if self.rank == 0 and not getattr(self, '_project_notice', False):
            print("--shapelet_project: the shapelets are now exact copies of training windows; for continued training, "
                  "IGN_TIE_EXACT=1 / model.set_tie_exact() gives the reference's sign(0) = 0 at x == w in the L1 backward "
                  "(not switched on automatically)")
        self._project_notice = True
        self._shapelet_sources = rep
        return rep

    def _project_final(self, best):
        """The projection after training: validation before and after it, the checkpoint re-saved with the same keys (rank 0) and
        shapelet_sources.json written beside it."""
        if self.args.model not in ('SBM', 'LTS', 'InterpGN'):
            self._project_shapelets()           # the notice; no validation pass for it
            return
        before = self._val_metrics()
        rep = self._project_shapelets()
        if rep is None:
            return
        after = self._val_metrics()
        if self.rank == 0:
            self._report_projection(rep, before, after, best)
        if self.distributed:
            dist.barrier()                      # the other ranks read the re-saved checkpoint next

    def _report_projection(self, rep, before, after, best):
        for g in rep["groups"]:
            d = g["d_before"][torch.isfinite(g["d_before"])]
            mean = float(d.double().mean()) if d.numel() else float('nan')
            print(f"shapelet_project: length {g['length']} mean d_before {mean:.6g} kept {g['kept']}")
        what = "accuracy" if before[1] is not None else "loss"
        pick = (lambda m: m[1]) if before[1] is not None else (lambda m: m[0])
        print(f"shapelet_project: validation {what} {pick(before):.4f} -> {pick(after):.4f} "
              f"({rep['samples']} training samples, {rep['batches']} batches)")
        from utils.shapelet_project import save_sources
        torch.save(self.model.state_dict(), best)
        save_sources(os.path.join(self.checkpoint_dir, 'shapelet_sources.json'), rep)

    def _shapelet_sources_for_test(self):
        """What test() reports about a projection: this run's report, else -- with the flag on, e.g. under --test_only -- the
        sidecar beside the checkpoint; None when nothing was projected."""
        rep = getattr(self, '_shapelet_sources', None)
        if rep is not None:
            return rep
        if self._project_schedule() == (0, False):
            return None
        path = os.path.join(self.checkpoint_dir, 'shapelet_sources.json')
        if not os.path.exists(path):
            return None
        from utils.shapelet_project import load_sources
        return load_sources(path)

    def _project_summary(self):
        """The summary CSV's columns of a run with --shapelet_project on (none: no column is added): the flag, and the mean
        distance between the shapelets and the windows that replaced them."""
        if self._project_schedule() == (0, False):
            return {}
        src = self._shapelet_sources_for_test()
        d = None if src is None else src["d_before"][torch.isfinite(src["d_before"])]
        return {'shapelet_project': str(self.args.shapelet_project),
                'project_d_mean': float(d.double().mean()) if d is not None and d.numel() else None}

    def _val_metrics(self):
        """-> (val_loss, val_accuracy or None) for the epoch loop of train()."""
        return self.validation()

    def validation(self):
        if len(self.val_loader) == 0:
            return float('inf'), 0.0
        a = self.args
        amp = a.amp and self.device.type == 'cuda'
        total, preds, trues = [], [], []
        self.model.eval()
        with torch.no_grad():
            for batch_x, label, padding_mask in self.val_loader:
                batch_x, label, padding_mask = self._to_device(batch_x, label, padding_mask)
                with torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=amp):
                    logits, info = self._forward(batch_x, padding_mask)
                    loss = F.cross_entropy(logits, label, reduction='none')
                    if a.model != 'DNN':
                        loss = loss + info.loss.mean()
                total.append(loss.flatten().float())
                preds.append(logits.float())
                trues.append(label)
        loss = torch.cat(total).mean().item()
        pred = torch.cat(preds).argmax(dim=1).cpu().numpy()
        acc = accuracy_score(pred, torch.cat(trues).flatten().cpu().numpy())
        self.model.train()
        return loss, acc

    def _explain_batches(self, loader):
        """The non-empty batches of `loader` (default: the test loader) on the device -> (batch_x, padding_mask): the one loop of
        the four explanation methods below."""
        for batch_x, label, padding_mask in (self.test_loader if loader is None else loader):
            if batch_x.size(0):
                batch_x, _, padding_mask = self._to_device(batch_x, label, padding_mask)
                yield batch_x, padding_mask

    @staticmethod
    def _on_host(parts, fields):
        """Per-batch results -> {field: its tensors concatenated over the batches on the host; None where the results hold None}"""
        return {k: None if getattr(parts[0], k) is None else torch.cat([getattr(p, k).cpu() for p in parts]) for k in fields}

    def saliency(self, loader=None, target=None, explain="sbm"):
        """Input saliency over `loader` (default: the test loader) -> one host tensor (N,T,C): per sample the gradient of a class
        logit w.r.t. the input series (utils.saliency.input_saliency; SBM / LTS / InterpGN).
        `target`: an int, or None for each sample's predicted class.  `explain`: "sbm" (the interpretable expert, the default),
        "gated" (the mixture an InterpGN with the FCN expert predicts with) or "dnn" (the FCN expert's logits)."""
        from utils.saliency import input_saliency
        out = [input_saliency(self.model, batch_x, target, explain=explain).cpu() for batch_x, _ in self._explain_batches(loader)]
        return torch.cat(out) if out else torch.empty(0, self.args.seq_len, self.args.enc_in)

    def evidence(self, loader=None, target=None, explain="sbm"):
        """Evidence maps over `loader` (default: the test loader) -> utils.evidence.Evidence of host tensors concatenated over the
        batches: per sample the share of a class logit that comes from every (time, electrode) through the shapelet expert (N,T,C),
        from every time step through the FCN expert (N,T) and from the bias (utils.evidence.evidence_map; SBM / LTS / InterpGN).
        `target`: an int, or None for each sample's predicted class.  `explain`: "sbm", "gated" (with --gating_value, as test
        applies it) or "dnn".  The loader's padding mask reaches the shapelet expert (--mask_padding)."""
        import dataclasses
        from utils.evidence import Evidence, evidence_map
        parts = [evidence_map(self.model, batch_x, target, explain=explain, gating_value=self.args.gating_value, mask=padding_mask)
                 for batch_x, padding_mask in self._explain_batches(loader)]
        return Evidence(**self._on_host(parts, [f.name for f in dataclasses.fields(Evidence)])) if parts else Evidence()

    def faithfulness(self, loader=None, target=None, **spec):
        """Deletion / insertion curves over `loader` (default: the test loader) -> utils.faithfulness.Faithfulness of host tensors
        concatenated over the batches, the summary numbers taken over all samples.  `spec`: the keyword arguments of
        utils.faithfulness.faithfulness_curves (explain, attributions, steps, mode, fill, unit, seed and, for the "occlusion"
        attribution, window, stride, groups; explain="model" serves whatever --model built); --gating_value is applied as
        test applies it and the loader's padding mask reaches the model (--mask_padding).  The random ranking of batch i is seeded
        with seed + i."""
        from utils.faithfulness import Faithfulness, concat, faithfulness_curves
        seed = int(spec.pop("seed", 0))
        parts = [faithfulness_curves(self.model, batch_x, mask=padding_mask, target=target, seed=seed + i,
                                     gating_value=self.args.gating_value, **spec)
                 for i, (batch_x, padding_mask) in enumerate(self._explain_batches(loader))]
        return concat(parts) if parts else Faithfulness()

    def occlusion(self, loader=None, target=None, **spec):
        """Occlusion maps over `loader` (default: the test loader) -> utils.occlusion.Occlusion of host tensors concatenated over the
        batches (map (N,T,C), drop (N,P), target (N,), base (N,)); every field None for an empty loader.  `spec`: the keyword
        arguments of utils.occlusion.occlusion_map (explain, window, stride, groups, fill, score, rows); explain="model" runs whatever
        --model built through utils.explain.model_logits, the calling convention of `_forward` at test time; --gating_value is
        applied as test applies it and the loader's padding mask reaches the model (--mask_padding)."""
        from utils.occlusion import Occlusion, occlusion_map
        parts = [occlusion_map(self.model, batch_x, mask=padding_mask, target=target, gating_value=self.args.gating_value, **spec)
                 for batch_x, padding_mask in self._explain_batches(loader)]
        return Occlusion(**self._on_host(parts, Occlusion._fields)) if parts else Occlusion()

    def test(self, save_csv=True, result_dir=None):
        """-> (test_loss, ClassificationResult, None)   (:828-1138; ``gating_value`` is applied here only)."""
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
            dnn_preds: list = field(default_factory=list)
            p: list = field(default_factory=list)
            d: list = field(default_factory=list)
            eta: list = field(default_factory=list)
            t: list = field(default_factory=list)
            loss: list = field(default_factory=list)

        buf = Buffer()       # accumulators stay ON THE DEVICE; one host copy per field after the loop
        self.model.eval()
        with torch.no_grad():
            for batch_x, label, padding_mask in self.test_loader:
                if batch_x.size(0) == 0:
                    continue
                batch_x, label, padding_mask = self._to_device(batch_x, label, padding_mask)
                ok = (label >= 0) & (label < a.num_class)           # drop out-of-range labels (:905-925)
                if not bool(ok.all()):
                    if not bool(ok.any()):
                        continue
                    batch_x, label, padding_mask = batch_x[ok], label[ok], padding_mask[ok]
                with torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=amp):
                    logits, info = self._forward(batch_x, padding_mask, gating_value=a.gating_value, test=True)
                    loss = F.cross_entropy(logits, label, reduction='none')
                    if a.model != 'DNN':
                        loss = loss + info.loss.mean()
                buf.loss.append(loss.flatten().float())
                buf.x_data.append(batch_x)
                buf.trues.append(label)
                buf.preds.append(logits.float())
                if a.model in ('InterpGN', 'SBM', 'LTS'):
                    buf.p.append(info.p)
                    buf.d.append(info.d)
                    buf.shapelet_preds.append(info.shapelet_preds.float())
                    if getattr(info, 't', None) is not None:
                        buf.t.append(info.t)
                    if a.model == 'InterpGN':
                        buf.eta.append(info.eta.float())
                        buf.dnn_preds.append(info.dnn_preds.float())
        if not buf.trues:
            return float('inf'), None, None
        host = lambda parts: torch.cat(parts).cpu()
        trues = host(buf.trues).flatten()
        logits = host(buf.preds)
        predictions = logits.argmax(dim=1)
        accuracy = accuracy_score(predictions.numpy(), trues.numpy())
        test_loss = torch.cat(buf.loss).mean().item()
        per_class = per_class_metrics(predictions, trues, a.num_class)
        if self.rank == 0:
            base = 100.0 / a.num_class
            print(f"Test: n={len(trues)} loss={test_loss:.6f} acc={accuracy:.4f} ({accuracy * 100:.2f}%; "
                  f"random baseline {base:.2f}%) balanced_acc={per_class['balanced_accuracy']:.4f} "
                  f"macro_f1={per_class['macro_f1']:.4f}")
        res = ClassificationResult(x_data=host(buf.x_data), trues=trues, preds=predictions, loss=test_loss,
                                   accuracy=accuracy, **per_class)
        if buf.p:
            res.p, res.d = host(buf.p), host(buf.d)
            if getattr(a, 'mask_padding', False):
                # ops.NO_WINDOW marks "no window": 0 for the score, which stays finite
                res.d = torch.where(res.d >= ign_ops.NO_WINDOW / 10, torch.zeros_like(res.d), res.d)
            res.shapelet_preds = host(buf.shapelet_preds)
            sbm = self.model.sbm if a.model == 'InterpGN' else self.model
            res.w = sbm.output_layer.weight.detach().cpu()
            res.shapelets = sbm.get_shapelets()
            if buf.t and hasattr(sbm, 'match_layout'):
                # where each shapelet matched each series: the forward kernel's arg-max window, as sample ranges
                stride, length = sbm.match_layout()
                res.t = host(buf.t)
                res.match_start, res.match_len = res.t * stride.unsqueeze(0), length
                if getattr(a, 'mask_padding', False):
                    # t = -1: the sample is shorter than the shapelet, there is no match to locate
                    none = res.t < 0
                    res.match_start = torch.where(none, torch.full_like(res.match_start, -1), res.match_start)
                    res.match_len = torch.where(none, torch.zeros_like(res.t), length.unsqueeze(0).expand_as(res.t))
            if a.model == 'InterpGN':
                res.eta = host(buf.eta)
                res.dnn_preds = host(buf.dnn_preds)
            src = self._shapelet_sources_for_test()
            if src is not None:                 # --shapelet_project: which training window every shapelet is a copy of
                res.shapelet_source, res.shapelet_source_start, res.shapelet_source_d = src["source"], src["start"], src["d_before"]
        test_df = None
        if save_csv and result_dir is not None and self.rank == 0:
            test_df = self._write_summary(res, result_dir)
        return test_loss, res, test_df

    SUMMARY_ARGS = ('model', 'dataset', 'dnn_type', 'train_epochs', 'num_shapelet', 'lambda_reg', 'lambda_div', 'epsilon', 'lr',
                    'seed', 'pos_weight', 'beta_schedule', 'gating_value', 'distance_func', 'sbm_cls', 'eeg_spatial')

    def _write_summary(self, res, result_dir):
        """One-row test summary: the run's hyper-parameters, accuracy, and -- for the shapelet models -- the
        interpretability statistics (gate mean / spread, shapelet score, sparsity and Gini index of the class weights).
        The reference intends exactly these columns (IGN/exp/experiment_classification.py:500-532) but its live ``test``
        leaves the CSV block empty (:1131-1136); written here with the file-name scheme of :530."""
        import csv
        from datetime import datetime
        a = self.args
        row = {k: getattr(a, k) for k in self.SUMMARY_ARGS if hasattr(a, k)}
        row['test_accuracy'] = res.accuracy
        row['epoch_stop'] = self.epoch_stop
        if a.model != 'DNN' and getattr(res, 'w', None) is not None:
            w = res.w.float()
            row['eta_mean'] = float(res.eta.mean()) if a.model == 'InterpGN' else None
            row['eta_std'] = float(res.eta.std()) if a.model == 'InterpGN' else None
            row['shapelet_score'] = compute_shapelet_score(res.d.float(), w, res.preds, res.trues)
            for thr in (1, 0.5, 0.1):
                big = (w.abs() > thr).float()
                row[f'w_count_{thr}'] = float(big.sum())
                row[f'w_ratio_{thr}'] = float(big.mean())
            row['w_max'] = float(w.abs().max())
            row['w_gini_clip'] = float(gini_coefficient(np.clip(w.numpy(), 0, None)))
            row['w_gini_abs'] = float(gini_coefficient(np.abs(w.numpy())))
        row.update(self._project_summary())
        stamp = datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
        path = os.path.join(result_dir, f"{a.dataset}-{a.seed}-{a.model}-{a.num_shapelet}-{a.lambda_div}-{a.lambda_reg}-{stamp}.csv")
        with open(path, "w", newline="") as f:
            wr = csv.DictWriter(f, fieldnames=list(row))
            wr.writeheader()
            wr.writerow(row)
        print(f"Test summary saved at: {path}")
        try:
            import pandas as pd
            return pd.DataFrame({k: [v] for k, v in row.items()})
        except ImportError:
            return row
