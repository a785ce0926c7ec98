"""Histogram counts and moments of device tensors, computed where the tensors live.

``DeviceSummarizer`` runs ``summary_stats`` (``csrc/kernels/summary.hip``) over segments of
fp32 / bf16 device tensors against TF's bucket limits and brings the results of a whole batch
of launches to the host in ONE copy: per segment ``len(BUCKET_LIMITS) + 1`` int32 counts and
four float64 moments (min, max, sum, sum of squares) instead of the tensors themselves.

A segment is ``(offset, rows, cols, row_stride)`` in elements of its source:
``src[offset + r * row_stride + c]`` for ``r < rows``, ``c < cols``; the columns from ``cols``
to ``row_stride`` are channel padding and are neither read into the result nor counted.
``counts[s, i]`` for ``i < NB`` is the number of finite values whose
``np.searchsorted(limits, v, side="left")`` is ``i``; column ``NB`` holds NaN, +-inf and
anything above the last limit, and those values stay out of the moments.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops._ext import kernels
from .events import BUCKET_LIMITS

Job = Tuple[torch.Tensor, Sequence[Sequence[int]], float]


class DeviceSummarizer:
    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceSummarizer needs a HIP device, got {self.device}")
        self.K = kernels()
        self.nb = int(BUCKET_LIMITS.size)
        self.limits = torch.from_numpy(BUCKET_LIMITS).to(self.device)    # the host table itself, uploaded once
        self._out: Optional[torch.Tensor] = None       # [stats of every segment | counts of every segment]
        self._scratch: Optional[torch.Tensor] = None
        self.copies = 0                                # D2H copies so far (one per run())

    def _buffers(self, nseg: int) -> Tuple[torch.Tensor, torch.Tensor]:
        need = nseg * 32 + nseg * (self.nb + 1) * 4
        if self._out is None or self._out.numel() < need:
            self._out = torch.empty(need, dtype=torch.uint8, device=self.device)
        ns = int(self.K.summary_scratch_size(nseg))
        if self._scratch is None or self._scratch.numel() < ns:
            self._scratch = torch.empty(ns, dtype=torch.float64, device=self.device)
        stats = self._out[:nseg * 32].view(torch.float64).view(nseg, 4)
        counts = self._out[nseg * 32:need].view(torch.int32).view(nseg, self.nb + 1)
        return counts, stats

    def run(self, jobs: Sequence[Job]) -> List[Tuple[np.ndarray, np.ndarray]]:
        """One launch set per job ``(src, segments, divisor)``; one copy to the host for all of
        them.  Returns per job ``(counts [nseg, NB + 1] int32, stats [nseg, 4] float64)``."""
        nsegs = [len(j[1]) for j in jobs]
        total = sum(nsegs)
        if total == 0:
            return [(np.zeros((0, self.nb + 1), np.int32), np.zeros((0, 4))) for _ in jobs]
        counts, stats = self._buffers(total)
        at = 0
        for (src, segs, divisor), n in zip(jobs, nsegs):
            if n:
                table = torch.tensor([[int(x) for x in s] for s in segs], dtype=torch.int64).view(n, 4)
                # every job writes its own rows; the scratch is reused (launches run in stream order)
                self.K.summary_stats(src, table, self.limits, counts[at:at + n], stats[at:at + n], self._scratch,
                                     float(divisor))
            at += n
        host = self._out[:total * 32 + total * (self.nb + 1) * 4].cpu().numpy()
        self.copies += 1
        h_stats = host[:total * 32].view(np.float64).reshape(total, 4)
        h_counts = host[total * 32:].view(np.int32).reshape(total, self.nb + 1)
        out, at = [], 0
        for n in nsegs:
            out.append((h_counts[at:at + n], h_stats[at:at + n]))
            at += n
        return out
