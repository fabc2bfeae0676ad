#!/usr/bin/env python3
"""CLI driver -- drop-in for IGN/run.py: every flag of IGN/run.py:17-135 with its default and meaning (including
the inverted ``--amp``: passing it turns bf16 autocast OFF), the seed loop ``[0,42,1234,8237,2023]``
(:564), checkpoint skip/load (:580-602), test + pickled results (:605-625).

Differences, all repairs of fork defects listed in SURVEY section 0:
  * ``--data`` defaults to ``UEA`` and ``--data_root`` to ``./data/UEA_multivariate`` (the upstream defaults that
    survive as comments in IGN/run.py:68-69), so ``run_uea.sh`` -- which passes neither -- works (D2);
  * ``--data SYNTH`` (+ ``--synthetic n,C,T,classes``) is the synthetic CHISCO-shaped provider of the benchmark;
  * ``--shapelet_init kmeans`` (+ ``--shapelet_init_iters``, ``--shapelet_init_batches``) starts the shapelets from k-means
    centroids of the training windows instead of N(0,1); the default ``normal`` is the reference's initialisation;
  * ``--shapelet_project none|end|N`` snaps every learned shapelet to the nearest real training window (after training, and with N
    also every N epochs before validation), re-saves the checkpoint and writes ``shapelet_sources.json`` beside it: per shapelet the
    data set index and first sample of the window it now is a bit-exact copy of; ``--test_only`` projects nothing and reads that
    file; the default ``none`` changes nothing;
  * ``--mask_padding`` makes the SBM / LTS expert normalise and match every sample of a ragged (zero-padded) batch over its own
    length only; the default, off, is the reference's behaviour (the padding takes part);
  * ``--class_weight none|balanced|w0,w1,...`` and ``--label_smoothing EPS`` turn the TRAINING cross-entropy into
    ``F.cross_entropy(weight=, label_smoothing=)`` (InterpGN: still one fused launch); validation / test losses stay plain CE;
  * ``--augment shift=0.1,scale=0.1,noise=0.05,chan_drop=0.1,time_mask=0.1`` (any subset) augments every TRAINING batch on the
    device in one fused launch: circular shift, per-channel gain, Gaussian noise, electrode dropout, one masked time span, each
    inside the sample's own length; validation / test never augment; the default ``none`` changes nothing;
  * ``--mix mixup=0.4[,cutmix=1][,prob=0.5]`` mixes every TRAINING sample with a partner of its batch on the device in one launch
    (mixup: a Beta(A, A) blend; cutmix: a time span of the partner) and trains on the soft labels (InterpGN: still one fused loss
    launch, also under ``--hipgraph``); classification only; validation / test never mix; the default ``none`` changes nothing;
  * ``--warp twarp=0.2[,mwarp=0.1][,wwarp=0.1][,knots=4][,prob=0.5]`` (any subset of the three rates) warps every TRAINING sample
    along time on the device in one launch, in front of ``--augment``: a smooth random speed curve (twarp), a smooth random gain
    curve shared by the channels (mwarp) and one window stretched or compressed by 2 (wwarp), each inside the sample's own length;
    classification and regression; validation / test never warp; the default ``none`` changes nothing;
  * ``--evidence sbm|gated|dnn`` writes ``evidence.npz`` beside the test results after the test: per test sample the predicted
    class's logit laid out over time and electrodes (the shapelet expert's (N,T,C) map, the FCN expert's (N,T) map and its bias),
    which sum to that logit, plus eta, logit, target and contrib (utils/evidence.py); needs ``--sbm_cls linear``; the default
    ``none`` imports and launches nothing;
  * ``--faithfulness explain=sbm|gated|dnn[,attr=evidence+saliency+random][,steps=10][,mode=deletion|insertion][,fill=mean|zero]
    [,unit=cell|time][,seed=0]`` writes ``faithfulness.json`` (the spec, the mean curves, AUC / AOPC / flip fraction per attribution
    and the gap to the random ranking) and ``faithfulness.npz`` (the per-sample curves) beside the test results after the test: the
    deletion / insertion test of the explanations (utils/faithfulness.py), ranking and perturbation on the device
    (``ign_rank_threshold``, ``ign_perturb_btc``); classification only; the default ``none`` parses, imports and launches nothing;
    ``explain=model`` with ``attr=occlusion+random`` (and ``window=``, ``stride=``, ``groups=``) draws the curves for every model;
  * ``--occlusion explain=model|sbm|gated|dnn[,window=W][,stride=S][,groups=all|each|PATH.npy][,fill=mean|zero][,score=logit|prob]
    [,rows=256]`` writes ``occlusion.npz`` beside the test results after the test: per test sample how far the predicted class's
    score falls when a window of time on a group of electrodes is hidden, laid back over the hidden cells (``map`` (N,T,C), ``drop``
    (N,P), ``target``, ``base``, ``gid`` and the grid; utils/occlusion.py) -- an attribution that needs a forward pass only, for
    every model (``explain=model``), head, distance and deep expert; the copies and the gather back run on the device
    (``ign_occlude_btc``, ``ign_occlusion_spread``); classification only; the default ``none`` parses, imports and launches nothing;
  * ``--eeg_preprocess band=8:30,decimate=2,fit`` (``--data EEG`` / ``EEG3``; any subset of sfreq=F, band=LO:HI, decimate=Q, taps=M,
    edge=reflect|zero, fit) filters the raw CHISCO shards with a zero-phase FIR band-pass, decimates them and, with ``fit``, crops /
    zero-pads them to ``--target_channels`` x ``--target_timepoints`` in front of the standardisation -- on the device in the
    prefetcher (two HIP passes), in numpy on the CPU item path; the default ``none`` changes nothing and leaves ``--target_*`` inert;
    ``bank=4:8+8:13+13:30+30:45`` (1 to 8 bands instead of ``band=``) makes a filter bank in the same two passes: every band of every
    electrode is a channel of its own, band-major (``enc_in`` = bands x electrodes; ``fit`` counts ``--target_channels`` per band),
    and ``envelope`` turns every band into its band-power envelope (needs ``edge=reflect`` and both edges of every band);
  * ``--eeg_spatial ref=car,matrix=PATH.npy,align=euclid`` (``--data EEG`` / ``EEG3``; any subset) applies one matrix per subject
    across the electrodes of the raw shards in front of all of that -- a common average reference, a montage or unmixing matrix
    computed offline, Euclidean alignment fitted on the training split -- as one exact-fp32 matrix-core launch in the prefetcher
    (numpy on the CPU item path); ``enc_in`` becomes the matrix's row count; the default ``none`` changes nothing;
  * ``--eeg_iir hp=0.5,lp=100,order=4,notch=50`` (``--data EEG`` / ``EEG3``; any subset) filters every row forward and backward
    along time with Butterworth and notch second-order sections (scipy's ``sosfiltfilt``, float64 recurrence) between
    ``--eeg_spatial`` and ``--eeg_preprocess``: drift and mains removal, which FIR taps cannot do inside a trial; shapes are kept;
    the default ``none`` changes nothing;
  * ``--eeg_resample rate=256`` (``--data EEG`` / ``EEG3``; or ``ratio=64/125``) changes the rate of every row by the exact fraction
    ``rate / sfreq`` with a polyphase Kaiser-windowed low-pass (scipy's ``resample_poly``) between ``--eeg_iir`` and
    ``--eeg_preprocess``: 500 -> 256 Hz, which ``decimate=Q`` cannot express; ``seq_len`` becomes ``ceil(T * up / down)``,
    ``--eeg_iir`` names the rate in front of it and ``--eeg_preprocess`` the rate behind it; the default ``none`` changes nothing;
  * ``--eeg_artifact clip=6,flat=0.01,noisy=8,neighbors=PATH.npy,report`` (``--data EEG`` / ``EEG3``; any subset) judges every row of the
    raw shards by its median and median absolute deviation in front of ``--eeg_spatial``: good rows are clamped to ``clip`` robust
    standard deviations, flat, noisy and non-finite electrodes are rebuilt from the good ones (``neighbors``: a (C, C) weight matrix),
    ``report`` counts the verdicts over the training split; nothing is dropped; the default ``none`` changes nothing;
  * the ``--eeg_*`` stages run in one fixed order: artifact -> spatial -> iir -> resample -> preprocess -> standardise
    (data_provider/eeg_chain.py);
  * ``--weight_decay WD``, ``--lr_schedule none|constant[,warmup=W]|cosine[,warmup=W][,min=M]`` and ``--ema D`` turn the flat Adam into
    AdamW with a per-optimizer-step schedule evaluated on the device and keep an exponential moving average of the weights that
    validation, early stopping and ``checkpoint.pth`` use (GPU only; all three default to off: the reference's optimizer);
  * ``--task_name regression --data Monash`` is the reference's regression twin (exp/experiment_regression.py), with the
    repairs R1-R3 of DESIGN 2.3;
  * multi-GPU is one process per GPU: ``python -m torch.distributed.run --nproc-per-node N run.py ...``.
"""
import argparse
import importlib
import os
import pickle
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np
import torch

from exp.experiment_classification import Experiment as ClassificationExperiment
from exp.experiment_regression import Experiment as RegressionExperiment

exp_dict = {
    "classification": ClassificationExperiment,
    "regression": RegressionExperiment,      # Monash TSER targets, binned, CRPS loss
}


def shapelet_project_arg(text):
    """--shapelet_project: 'none', 'end' or an integer N >= 1 (-> int)."""
    if text in ('none', 'end'):
        return text
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError(f"expected none, end or an integer N >= 1, got {text!r}")
    return n


def build_parser():
    p = argparse.ArgumentParser()
    # data
    p.add_argument("--data", type=str, default="UEA", choices=['EEG', 'EEG3', 'UEA', 'SYNTH', 'Monash'])
    p.add_argument("--data_root", type=str, default="./data/UEA_multivariate")
    p.add_argument("--json_path", type=str, default="./json/textmaps.json")
    p.add_argument("--hipgraph", action="store_true",
                   help="replay the training step (forward, fused loss, backward, Adam) as one captured hipGraph -- for the "
                        "launch-bound regime of small batches (run_uea.sh: --batch_size 32): one host call per step instead of "
                        "~45 launches.  Ignored (eager) with gradient accumulation / clipping, bf16 autocast or several ranks")
    p.add_argument("--synthetic", type=str, default=None, help="SYNTH provider: n,C,T,classes (default 8192,122,1000,3)")
    p.add_argument("--target_channels", type=int, default=122)
    p.add_argument("--target_timepoints", type=int, default=1651)
    p.add_argument("--max_files", type=int, default=1000)
    p.add_argument("--max_subjects", type=int, default=5)
    p.add_argument("--subject_id", type=str, default="sub-01")
    p.add_argument("--subject_ids", type=str, nargs='+', default=["sub-01,sub-02,sub-03"])
    p.add_argument("--task_type", type=str, default="imagine", choices=['imagine', 'read', 'both'])
    # EEG-CNN baseline
    p.add_argument("--eegcnn_layers", type=int, default=2)
    p.add_argument("--eegcnn_pooling", type=str, default='mean', choices=[None, 'mean', 'sum', 'top'])
    p.add_argument("--eegcnn_cnn_f1", type=int, default=8)
    p.add_argument("--eegcnn_cnn_f2", type=int, default=8)
    p.add_argument("--eegcnn_kernel1", type=int, default=125)
    p.add_argument("--eegcnn_kernel2", type=int, default=25)
    p.add_argument("--eegcnn_pool1", type=int, default=2)
    p.add_argument("--eegcnn_pool2", type=int, default=5)
    p.add_argument("--eegcnn_dropout1", type=float, default=0.1)
    p.add_argument("--eegcnn_dropout2", type=float, default=0.1)
    p.add_argument("--eegcnn_n_heads", type=int, default=8)
    p.add_argument("--eegcnn_d_ff", type=int, default=256)
    # SBM / InterpGN
    p.add_argument("--model", type=str, default='InterpGN', choices=['SBM', 'LTS', 'InterpGN', 'DNN', 'EEGCNN'])
    p.add_argument("--dnn_type", type=str, default='Transformer',
                   choices=['FCN', 'Transformer', 'TimesNet', 'PatchTST', 'ResNet'])
    p.add_argument("--dataset", type=str, default="BasicMotions")
    p.add_argument("--lambda_reg", type=float, default=0.1)
    p.add_argument("--lambda_div", type=float, default=0.1)
    p.add_argument("--epsilon", type=float, default=1.)
    p.add_argument("--num_shapelet", type=int, default=10)
    p.add_argument("--gating_value", type=float, default=None)
    p.add_argument("--pos_weight", action="store_true")
    p.add_argument("--sbm_cls", type=str, default='linear')
    p.add_argument("--distance_func", type=str, default='euclidean')
    p.add_argument("--beta_schedule", type=str, default='constant')
    p.add_argument("--memory_efficient", action="store_true")
    p.add_argument("--shapelet_init", type=str, default='normal', choices=['normal', 'kmeans'],
                   help="normal: N(0,1) shapelets as the reference; kmeans: k-means centroids of the training windows "
                        "(utils/shapelet_init.py; SBM / LTS / InterpGN, before training)")
    p.add_argument("--shapelet_init_iters", type=int, default=10, help="Lloyd iterations of --shapelet_init kmeans")
    p.add_argument("--shapelet_init_batches", type=int, default=8, help="training batches --shapelet_init kmeans clusters")
    p.add_argument("--shapelet_project", type=shapelet_project_arg, default='none', metavar="none|end|N",
                   help="snap every shapelet of an SBM / LTS / InterpGN model to the nearest real training window under the model's "
                        "own distance (utils/shapelet_project.py) and record where it came from.  end: after the best checkpoint is "
                        "reloaded -- validation before / after is printed, checkpoint.pth is re-saved with the same keys and "
                        "shapelet_sources.json (group, k, c, data set index, start, length, distance per feature column) is written "
                        "beside it.  N >= 1: also after the training pass of every N-th epoch, before its validation, so early "
                        "stopping and the checkpoint see a projected model; Adam's moments are left alone.  One ordered, "
                        "un-augmented pass over the whole training set on every rank (no collective).  none: off")
    p.add_argument("--mask_padding", action="store_true",
                   help="variable-length series: the SBM / LTS expert takes instance norm, shapelet matches and match locations over "
                        "each sample's own length (the loader's padding mask) instead of over the zero padding.  Off: the "
                        "reference's behaviour.  Trains eagerly (no --hipgraph); not with --shapelet_init kmeans")
    p.add_argument("--class_weight", type=str, default='none',
                   help="class weights of the training cross-entropy: none; balanced = n / (classes present * count_c) from the "
                        "training labels; or one positive value per class, w0,w1,...  Validation / test losses stay unweighted")
    p.add_argument("--label_smoothing", type=float, default=0.0, help="label smoothing of the training cross-entropy, in [0, 1)")
    p.add_argument("--augment", type=str, default='none',
                   help="training-batch augmentation on the device, one fused launch per step: none, or a comma list of "
                        "shift=R (circular shift by up to R * length), scale=R (per-channel gain in 1 +- R; the SBM's instance norm "
                        "cancels it, the DNN experts see it), noise=SIGMA (Gaussian), chan_drop=P (electrodes zeroed, no rescaling), "
                        "time_mask=R (one zeroed span of up to R * length per sample); rates in [0, 1).  Reproducible from --seed")
    p.add_argument("--mix", type=str, default='none',
                   help="mixup / CutMix of the training batch on the device, one launch per step, with soft labels through the loss: "
                        "none, or mixup=A[,cutmix=A][,prob=P].  A > 0 is the Beta(A, A) parameter of the mixing share; cutmix "
                        "replaces one time span of a sample by its partner's instead of blending; with both keys each mixed sample "
                        "takes one of the two with probability 1/2; prob in (0, 1] is the chance that a sample is mixed at all.  "
                        "Partners are a random roll of the batch.  Classification only.  Reproducible from --seed")
    p.add_argument("--warp", type=str, default='none',
                   help="time, magnitude and window warping of the training batch on the device, one launch per step in front of "
                        "--augment: none, or twarp=R[,mwarp=R][,wwarp=R][,knots=K][,prob=P] with any subset of the three rates.  "
                        "twarp=R resamples every sample through a smooth monotone time map whose local speed lies in 1 +- R; mwarp=R "
                        "multiplies it by a smooth gain curve in 1 +- R, one curve for all channels; wwarp=R stretches or compresses "
                        "one window of R * length by 2 and rescales the sample to its length; rates in [0, 1).  knots=K (1..8, "
                        "default 4) interior knots of the two curves; prob in (0, 1] is the chance that a sample is warped at all.  "
                        "Reproducible from --seed")
    p.add_argument("--evidence", type=str, default='none', choices=('none', 'sbm', 'gated', 'dnn'),
                   help="after the test, write evidence.npz beside the test results: per test sample the share of the predicted "
                        "class's logit that comes from every (time, electrode) through the shapelet expert (sbm, (N,T,C)), from "
                        "every time step through the FCN expert (dnn, (N,T)) and from its bias (remainder), which sum to the logit; "
                        "plus eta, logit, target and contrib = W[target] * p, the reference's ranking key of the shapelets.  sbm: the "
                        "interpretable expert of SBM / LTS / InterpGN; dnn: the FCN expert; gated: the mixture InterpGN predicts "
                        "with, --gating_value applied.  Needs --sbm_cls linear (the other heads are not additive in p)")
    p.add_argument("--faithfulness", type=str, default='none',
                   help="after the test, write faithfulness.json and faithfulness.npz beside the test results: deletion / insertion "
                        "curves of the explanations over the test set.  none, or explain=sbm|gated|dnn followed by any of "
                        "attr=evidence+saliency+random (the rankings compared), steps=N (1..31 fractions j/N, default 10), "
                        "mode=deletion|insertion, fill=mean|zero (what replaces a cell: its electrode's mean over the sample, or "
                        "0), unit=cell|time (rank cells, or whole time steps), seed=S (of the random ranking).  evidence needs "
                        "--sbm_cls linear; saliency refuses what input gradients refuse.  attr may also name occlusion (see "
                        "--occlusion; its grid is window=W, stride=S, groups=all|each|PATH.npy), and explain=model with "
                        "attr=occlusion+random draws the curves for any model, head and distance.  Classification only")
    p.add_argument("--occlusion", type=str, default='none',
                   help="after the test, write occlusion.npz beside the test results: occlusion maps over the test set.  none, or "
                        "explain=model|sbm|gated|dnn (model: whatever --model built, as the test runs it; the rest as --evidence) "
                        "followed by any of window=W, stride=S (time steps; 0 = the whole series / the window), "
                        "groups=all|each|PATH.npy (electrodes hidden together: all of them, one at a time, or an int array (C,) of "
                        "group ids), fill=mean|zero, score=logit|prob, rows=R (occluded copies per forward, default 256).  Works "
                        "for every model, head and distance.  Classification only")
    p.add_argument("--eeg_preprocess", type=str, default='none',
                   help="--data EEG / EEG3: preprocessing of the raw shards in front of the standardisation, on the device: none, or a "
                        "comma list of sfreq=F (Hz, default 500), band=LO:HI (Hz, either side may be empty), decimate=Q, taps=M "
                        "(odd, <= 1023; default 20Q+1 when only decimating, else 3.3*sfreq/lowest edge), edge=reflect|zero, and fit "
                        "(output shape --target_channels x --target_timepoints, cropped / zero-padded and masked; without it "
                        "channels x ceil(T/Q)).  A zero-phase Hamming windowed-sinc FIR filter; an upper edge above sfreq/(2Q) is "
                        "refused.  bank=LO:HI+LO:HI+... (1 to 8 bands, instead of band=; one tap count for all) gives a filter bank: "
                        "band-major channels, channel j*C + c is electrode c of band j, and fit then means --target_channels "
                        "electrodes per band; envelope replaces every band by its amplitude envelope (Hilbert-pair FIR; needs "
                        "edge=reflect and both edges of every band; band=LO:HI,envelope is a bank of one band).  --augment sees the "
                        "bank's channels: its chan_drop drops single band channels, not whole electrodes")
    p.add_argument("--eeg_spatial", type=str, default='none',
                   help="--data EEG / EEG3: a spatial filter across the electrodes of the raw shards, in front of --eeg_preprocess and "
                        "the standardisation, one matrix-core launch on the device: none, or a comma list of ref=car (common average "
                        "reference), matrix=PATH.npy (a (Cs,C) montage / unmixing matrix computed offline, or (G,Cs,C) with one per "
                        "subject), align=euclid (Euclidean alignment: every subject's trials whitened by the inverse square root of "
                        "that subject's mean spatial covariance, fitted on the training split before the first step) and rtol=R "
                        "(default 1e-6: eigenvalues below R times the largest are not inverted).  The matrices compose as "
                        "align . matrix . ref; the models see Cs virtual channels.  Subjects come from the optional <root>/subject.npy "
                        "(n,) integer ids; without it all trials are one group.  What was applied is written as eeg_spatial.npz beside "
                        "the checkpoint")
    p.add_argument("--eeg_iir", type=str, default='none',
                   help="--data EEG / EEG3: a zero-phase IIR stage along time on every row of the raw shards, behind --eeg_spatial and in "
                        "front of --eeg_preprocess and the standardisation, one launch on the device (float64 recurrence): none, or a "
                        "comma list of hp=F and lp=F (Butterworth high-pass / low-pass edges in Hz), order=N (1..8, default 4, of hp "
                        "and of lp each), notch=F[+F...] (notch centres in Hz), q=Q (default 30: each notch is F/Q Hz wide), sfreq=F "
                        "(default 500; must equal --eeg_preprocess's) and pad=P (samples of odd extension on both sides; default "
                        "scipy's 3 * (2 * sections + 1 - first-order sections)).  Sections run hp, lp, notches, forward then backward "
                        "(scipy.signal.sosfiltfilt); at most 8 sections; shapes do not change.  What was applied is written as "
                        "eeg_iir.json beside the checkpoint")
    p.add_argument("--eeg_resample", type=str, default='none',
                   help="--data EEG / EEG3: a rational change of the sampling rate along time on every row of the raw shards, behind "
                        "--eeg_iir and in front of --eeg_preprocess and the standardisation, one launch on the device: none, or a "
                        "comma list of rate=F (the output rate in Hz) or ratio=P/Q in its place, sfreq=F (the input rate, default 500; "
                        "--eeg_iir must name it, --eeg_preprocess must name the output rate), half=H (1..32, default 10: the low-pass "
                        "reaches H * max(up, down) samples of the up-sampled grid to each side), beta=B (of its Kaiser window, default "
                        "5.0) and edge=reflect|zero (default reflect).  up/down is the exact fraction rate/sfreq (256/500 = 64/125); "
                        "rows of T samples leave with ceil(T * up / down); the filter is scipy.signal.resample_poly's, applied to "
                        "the row minus its first sample.  What was applied is written as eeg_resample.json beside the checkpoint")
    p.add_argument("--eeg_artifact", type=str, default='none',
                   help="--data EEG / EEG3: an artifact stage on every row of the raw shards, in front of --eeg_spatial, three launches "
                        "on the device: none, or a comma list of clip=K (good rows are clamped to their median +- K * 1.4826 * MAD), "
                        "flat=F (in [0, 1): an electrode whose MAD is at most F times the trial's median MAD is flat), noisy=N (> 1: "
                        "one whose MAD is above N times it is noisy), neighbors=PATH.npy (a (C,C) non-negative weight matrix, e.g. "
                        "inverse electrode distances; default: all ones) and report (count the verdicts over the training split "
                        "before the first step and print the worst electrodes).  Flat, noisy and non-finite electrodes are rebuilt "
                        "as the weighted mean of the trial's good electrodes about their medians; a trial without a good electrode "
                        "is left clamped.  Medians are lower medians (exact order statistics).  Trials are never dropped.  What was "
                        "applied, and the report, is written as eeg_artifact.json beside the checkpoint")
    # experiment
    p.add_argument("--lr", type=float, default=5e-3)
    p.add_argument("--lr_decay", action="store_true")
    p.add_argument("--weight_decay", type=float, default=0.0,
                   help="decoupled weight decay as torch.optim.AdamW: p *= 1 - lr_t * WD in front of the Adam update, on the flat "
                        "optimizer path (GPU).  Matrices and convolution kernels decay; biases, BatchNorm / LayerNorm parameters, the "
                        "shapelet banks and the LTS thresholds do not.  0: plain Adam, as the reference")
    p.add_argument("--lr_schedule", type=str, default='none', metavar="none|constant[,warmup=W]|cosine[,warmup=W][,min=M]",
                   help="learning rate per OPTIMIZER STEP, computed on the device (one --hipgraph capture serves the run): linear "
                        "warm-up base * s / W over the first W steps, then constant, or a cosine from --lr down to M at the run's "
                        "last step (CosineAnnealingLR's closed form over train_epochs * batches // accumulation - W steps).  Not "
                        "with --lr_decay.  none: the reference's behaviour")
    p.add_argument("--ema", type=float, default=0.0, metavar="D",
                   help="exponential moving average of the parameters, decay D in [0, 1) (e.g. 0.999; warmed up as "
                        "min(D, (1 + s) / (10 + s))): validation, early stopping and checkpoint.pth use the averaged weights, "
                        "training goes on with the live ones; BatchNorm running statistics are the live ones.  Not with "
                        "--shapelet_project N.  0: off")
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--gradient_clip", type=float, default=0)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument('--log_interval', type=int, default=20)
    p.add_argument("--min_epochs", type=int, default=0)
    p.add_argument("--train_epochs", type=int, default=500)
    p.add_argument("--num_workers", type=int, default=0)
    p.add_argument("--patience", type=int, default=50)
    p.add_argument("--multi_gpu", action='store_true')
    p.add_argument("--test_only", action='store_true')
    p.add_argument("--seed", type=int, default=-1)
    p.add_argument("--amp", action='store_false', default=True)     # sic: the flag turns autocast OFF (D3)
    # basic config
    p.add_argument('--task_name', type=str, default='classification')
    p.add_argument('--model_id', type=str, default='test')
    p.add_argument('--embed', type=str, default='timeF')
    p.add_argument('--freq', type=str, default='h')
    # DNN configs
    p.add_argument('--top_k', type=int, default=5)
    p.add_argument('--num_kernels', type=int, default=6)
    p.add_argument('--enc_in', type=int, default=7)
    p.add_argument('--dec_in', type=int, default=7)
    p.add_argument('--c_out', type=int, default=7)
    p.add_argument('--d_model', type=int, default=512)
    p.add_argument('--n_heads', type=int, default=8)
    p.add_argument('--e_layers', type=int, default=2)
    p.add_argument('--d_layers', type=int, default=1)
    p.add_argument('--d_ff', type=int, default=2048)
    p.add_argument('--moving_avg', type=int, default=25)
    p.add_argument('--factor', type=int, default=1)
    p.add_argument('--distil', action='store_false', default=True)
    p.add_argument('--dropout', type=float, default=0)
    p.add_argument('--activation', type=str, default='gelu')
    p.add_argument('--output_attention', action='store_true')
    p.add_argument('--label_len', type=int, default=48)
    p.add_argument('--pred_len', type=int, default=96)
    p.add_argument('--seasonal_patterns', type=str, default='Monthly')
    p.add_argument('--inverse', action='store_true', default=False)
    return p


def check_args(args):
    """Combinations of flags that are refused before anything is built."""
    if getattr(args, 'mask_padding', False) and getattr(args, 'shapelet_init', 'normal') == 'kmeans':
        raise ValueError("--shapelet_init kmeans with --mask_padding: k-means would cluster windows of the zero padding "
                         "(there is no length-aware k-means step); use --shapelet_init normal")
    from utils.class_weight import check_loss_options
    check_loss_options(args, _num_class_from_flags(args))
    from utils.train_transforms import parse_flags
    parse_flags(args)                               # --warp / --augment / --mix, and --mix with the regression task
    for flag, parser, follows, _ in EXPLAIN_FLAGS:
        if parser is not None and _flag_on(args, flag):
            module, _, name = parser.rpartition('.')
            getattr(importlib.import_module(module), name)(getattr(args, flag))
            if getattr(args, 'task_name', 'classification') != 'classification':
                raise ValueError(f"--{flag} with --task_name regression: {follows}; classification only")
    from data_provider.eeg_chain import EEGChain
    EEGChain.from_args(args).check(getattr(args, 'data', None))      # the --eeg_* flags: the data they need, the rates they name
    from utils.optim_rule import check_optim_options
    check_optim_options(args, flat_path=torch.cuda.is_available())


def _num_class_from_flags(args):
    """The class count where the flags alone fix it (SYNTH, the 3-class CHISCO fold), else None: the dataset decides, and Experiment
    repeats the check of an explicit --class_weight list against it."""
    if getattr(args, 'data', None) == 'SYNTH':
        return int((getattr(args, 'synthetic', None) or "8192,122,1000,3").split(',')[3])
    return 3 if getattr(args, 'data', None) == 'EEG3' else None


def get_args(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    args.root_path = args.data_root if args.data in ('EEG', 'EEG3', 'SYNTH') else f"{args.data_root}/{args.dataset}"
    args.is_training = True
    return args


def set_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


def init_distributed():
    """One process per GPU when launched by torch.distributed.run; RCCL ('nccl') over xGMI."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0
    import torch.distributed as dist
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group("gloo")
    return dist.get_rank()


def main(argv=None):
    args = get_args(argv)
    exp_cls = exp_dict.get(args.task_name)
    if exp_cls is None:
        raise SystemExit(f"task_name={args.task_name!r} is not part of this build")
    rank = init_distributed()
    if args.data in ('EEG', 'EEG3', 'UEA', 'Monash') and not os.path.exists(args.root_path):
        raise SystemExit(f"data path does not exist: {args.root_path}")
    seeds = [0, 42, 1234, 8237, 2023] if args.seed == -1 else [args.seed]
    for i, seed in enumerate(seeds):
        set_seed(seed)
        args.seed = seed
        print(f"===== experiment {i + 1}/{len(seeds)} - seed {seed} =====")
        experiment = exp_cls(args=args)
        if rank == 0:
            experiment.print_args()
        ckpt = f"{experiment.checkpoint_dir}/checkpoint.pth"
        if not args.test_only:
            if os.path.exists(ckpt):
                print(f"checkpoint exists, skipping training: {ckpt}")
            else:
                experiment.train()
                torch.cuda.empty_cache()
        elif not os.path.exists(ckpt):
            print(f"warning: checkpoint missing, nothing to test: {ckpt}")
            continue
        if os.path.exists(ckpt):
            experiment.model.load_state_dict(torch.load(ckpt, map_location=experiment.device, weights_only=True))
        else:
            print("warning: testing a randomly initialised model")
        test_loss, test_metrics, test_df = experiment.test(save_csv=True, result_dir=f"./result/{args.model}")
        if rank == 0 and args.task_name == 'regression':
            with open(f"{os.path.dirname(ckpt)}/test_results.pkl", 'wb') as f:
                pickle.dump({'test_loss': test_loss, 'test_df': test_df, 'args': vars(args)}, f)
            print(f"CRPS: {test_loss:.6f}")
        elif rank == 0 and test_metrics is not None:
            with open(f"{os.path.dirname(ckpt)}/test_results.pkl", 'wb') as f:
                pickle.dump({'test_loss': test_loss, 'test_metrics': test_metrics, 'test_df': test_df,
                             'args': vars(args)}, f)
            print(f"accuracy: {test_metrics.accuracy:.4f}  loss: {test_metrics.loss:.4f}")
        for flag, _, _, writer in EXPLAIN_FLAGS:
            if rank == 0 and _flag_on(args, flag):
                writer(experiment, getattr(args, flag), os.path.dirname(ckpt))


def write_evidence(experiment, explain, path):
    """--evidence: the maps of Experiment.evidence over the test set as one .npz (the fields of utils.evidence.Evidence that apply)."""
    import dataclasses
    ev = experiment.evidence(explain=explain)
    arrays = {f.name: getattr(ev, f.name).numpy() for f in dataclasses.fields(ev) if getattr(ev, f.name) is not None}
    np.savez(path, **arrays)
    print(f"evidence ({explain}): {', '.join(f'{k} {v.shape}' for k, v in arrays.items())} -> {path}")


def write_faithfulness(experiment, spec, out_dir):
    """--faithfulness: the curves of Experiment.faithfulness over the test set as faithfulness.json (spec, mean curves, summary
    numbers) and faithfulness.npz (per-sample curves)."""
    import json
    from utils.faithfulness import parse_faithfulness, to_arrays, to_json
    spec = parse_faithfulness(spec)
    f = experiment.faithfulness(**spec._asdict())
    if f.target is None:
        print("faithfulness: the test loader is empty, nothing written")
        return
    with open(f"{out_dir}/faithfulness.json", 'w') as fh:
        json.dump(to_json(f, spec), fh, indent=1, sort_keys=True)
    np.savez(f"{out_dir}/faithfulness.npz", **to_arrays(f))
    print(f"faithfulness ({spec.explain}, {spec.mode}, {f.target.shape[0]} samples): " +
          ', '.join(f'{a}: auc {f.auc[a]:.4f} aopc {f.aopc[a]:.4f} flip {f.flip[a]:.3f}' for a in f.auc) + f" -> {out_dir}")


def write_occlusion(experiment, spec, path):
    """--occlusion: the maps of Experiment.occlusion over the test set as one .npz (map, drop, target, base, gid and the grid)."""
    from utils.occlusion import parse_occlusion, to_arrays
    spec = parse_occlusion(spec)
    occ = experiment.occlusion(**spec._asdict())
    if occ.map is None:
        print("occlusion: the test loader is empty, nothing written")
        return
    arrays = to_arrays(occ, spec, occ.map.shape[1], occ.map.shape[2])
    np.savez(path, **arrays)
    print(f"occlusion ({spec.explain}, {int(arrays['windows'])} windows x {int(arrays['groups'])} groups, {occ.map.shape[0]} samples): "
          f"{', '.join(f'{k} {v.shape}' for k, v in arrays.items())} -> {path}")


def _flag_on(args, flag):
    return str(getattr(args, flag, 'none')).strip().lower() != 'none'


# The explanation flags that act after the test, in the order they are served: (flag, its parser -- imported only when the flag is on
# -- or None: argparse's choices check it, what a regression run is told, writer(experiment, the flag's value, the checkpoint's folder)).
EXPLAIN_FLAGS = (
    ("evidence", None, None, lambda experiment, explain, out_dir: write_evidence(experiment, explain, f"{out_dir}/evidence.npz")),
    ("faithfulness", "utils.faithfulness.parse_faithfulness", "the curves follow a class logit", write_faithfulness),
    ("occlusion", "utils.occlusion.parse_occlusion", "the maps follow a class score",
     lambda experiment, spec, out_dir: write_occlusion(experiment, spec, f"{out_dir}/occlusion.npz")),
)


if __name__ == "__main__":
    main()
