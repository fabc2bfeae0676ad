"""Datasets behind ``data_dict`` (contract of IGN/data_factory/data_loader.py:600-719 for UEA, :722-856 for Monash).

The classification and regression paths of the reference are in scope; forecasting / anomaly loaders
(ETT, M4, PSM ...) are not rebuilt.
"""
import glob
import os
import re

import numpy as np
import torch
from torch.utils.data import Dataset

from data_provider.ts_reader import load_ts
from data_provider.uea import Normalizer, interpolate_missing, subsample, subsample_stride


class UEAloader(Dataset):
    """UEA multivariate archive ``<root>/<Dataset>_{TRAIN,TEST}.ts``.

    Items are ``(x[T_i, C] float64 tensor, label[1] int8 tensor)`` like the reference; ``collate_fn`` pads
    them to ``args.seq_len``.  Attributes the harness reads: ``max_seq_len``, ``feature_df`` (rows x C array),
    ``class_names`` -- plus ``seq_len / enc_in / num_classes`` so ``_get_params_from_data`` does not fall
    through to its EEG defaults.  ``flag`` is matched case-insensitively and 'val' maps to the
    TEST file, which is what upstream does.
    """
    label_dtype = np.int8

    def __init__(self, root_path, file_list=None, limit_size=None, flag=None):
        self.root_path = root_path
        series, codes = self.load_all(root_path, file_list=file_list, flag=flag)
        if limit_size is not None:
            n = int(limit_size) if limit_size > 1 else int(limit_size * len(series))
            series, codes = series[:n], codes[:n]
        self.all_IDs = np.arange(len(series))
        self.labels_df = np.asarray(codes, dtype=self.label_dtype).reshape(-1, 1)
        lengths = np.array([s.shape[0] for s in series])
        ids = np.repeat(self.all_IDs, lengths)
        stacked = np.concatenate(series, axis=0)
        self.feature_df = Normalizer().normalize(stacked, ids)          # standardise over all rows (uea.py:85-89)
        self._offsets = np.concatenate([[0], np.cumsum(lengths)])
        self.feature_names = [f"dim_{i}" for i in range(stacked.shape[1])]
        self.enc_in = stacked.shape[1]
        self.seq_len = int(self.max_seq_len)
        self.num_classes = len(self.class_names)
        print(len(self.all_IDs))

    def load_all(self, root_path, file_list=None, flag=None):
        paths = glob.glob(os.path.join(root_path, '*')) if file_list is None else \
            [os.path.join(root_path, p) for p in file_list]
        if not paths:
            raise Exception('No files found using: {}'.format(os.path.join(root_path, '*')))
        if flag is not None:
            want = 'TRAIN' if flag.lower() == 'train' else 'TEST'
            paths = [p for p in paths if re.search(want, os.path.basename(p), re.IGNORECASE)]
        paths = sorted(p for p in paths if os.path.isfile(p) and p.endswith('.ts'))
        if not paths:
            raise Exception("No .ts files found using pattern: '*.ts'")
        return self.load_single(paths[0])

    def load_single(self, filepath):
        cases, labels, _ = load_ts(filepath)
        if labels is None:
            raise Exception(f"{filepath}: no class labels")
        self.class_names = sorted(set(labels))
        codes = [self.class_names.index(l) for l in labels]
        return self._assemble(cases), codes

    def _assemble(self, cases):
        """ragged-dimension subsampling, max_seq_len and missing-value interpolation -> list of (T_i, C) float64 arrays"""
        lens = np.array([[len(d) for d in c] for c in cases])
        if np.abs(lens - lens[:, :1]).sum() > 0:          # dimensions of one case differ in length
            cases = [[subsample(d) for d in c] for c in cases]
            lens = np.array([[len(d) for d in c] for c in cases])
        self.max_seq_len = int(lens[:, 0].max())
        series = []
        for c in cases:
            n = len(c[0])
            arr = np.stack([interpolate_missing(np.asarray(d[:n], dtype=np.float64)) if len(d) >= n
                            else interpolate_missing(np.pad(np.asarray(d, dtype=np.float64), (0, n - len(d)),
                                                            constant_values=np.nan)) for d in c], axis=1)
            series.append(arr)                             # (T_i, C)
        return series

    def instance_norm(self, case):
        if self.root_path.count('EthanolConcentration') > 0:      # data_loader.py:705-713
            case = case - case.mean(0, keepdim=True)
            return case / torch.sqrt(torch.var(case, dim=1, keepdim=True, unbiased=False) + 1e-5)
        return case

    def __getitem__(self, ind):
        lo, hi = self._offsets[ind], self._offsets[ind + 1]
        return self.instance_norm(torch.from_numpy(self.feature_df[lo:hi])), torch.from_numpy(self.labels_df[ind])

    def __len__(self):
        return len(self.all_IDs)


class Monashloader(UEAloader):
    """Monash TSER regression archive ``<root>/<Dataset>_{TRAIN,TEST}.ts`` (``@targetLabel true``): UEAloader's rules for
    the series (ragged dimensions, missing values, standardisation over all rows), real-valued targets binned for the
    CRPS loss (IGN/data_factory/data_loader.py:798-810).

    Items are ``(x[T_i, C] float64, target[1] float32)`` -- the target stays real-valued (repair R1: the reference
    truncates it with ``.long()``).  ``bin_edges`` (float64, nbins values): the upper edges of ``nbins`` equal-width bins
    over the TRAIN targets, the last one +inf; val / test receive the train split's edges.  ``class_names`` is
    ``bin_edges``, so ``num_classes == nbins``.  ``stride`` / ``seq_len``: one fixed subsampling stride for every batch,
    ``ceil(max_seq_len / 1000)`` from 1000 samples on, and the subsampled length (repair R2).
    """
    label_dtype = np.float32

    def __init__(self, root_path, flag=None, bin_edges=None, nbins=10, file_list=None, limit_size=None):
        self.nbins = int(nbins)
        self.bin_edges = None if bin_edges is None else np.asarray(bin_edges, dtype=np.float64).reshape(-1)
        super().__init__(root_path, file_list=file_list, limit_size=limit_size, flag=flag)
        self.stride = subsample_stride(self.max_seq_len)
        self.seq_len = len(range(0, self.max_seq_len, self.stride))

    def load_single(self, filepath):
        cases, labels, _ = load_ts(filepath)
        if labels is None:
            raise Exception(f"{filepath}: no regression targets (@targetLabel true)")
        y = np.array([float(v) for v in labels], dtype=np.float64)     # a file with class labels too: numeric names
        if self.bin_edges is None:
            edges = np.linspace(y.min(), y.max(), self.nbins + 1)
            edges[0], edges[-1] = -np.inf, np.inf
            self.bin_edges = edges[1:]
        self.class_names = self.bin_edges
        return self._assemble(cases), y
