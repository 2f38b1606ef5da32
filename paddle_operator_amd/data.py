"""Token files and the replayable window sampler of the GPT-2 trainer.

**File format.**  Raw little-endian ``uint16`` token ids, no header (nanoGPT's
``train.bin`` / ``val.bin``): ``n = size / 2`` tokens.  An odd size, a file of
fewer than ``S + 1`` tokens and a model whose ``vocab_size`` exceeds 65536 are
rejected.

**Sampler.**  Counter-based like the dropout masks (``csrc/hip/philox.h``): the
windows of micro-batch ``m`` are a pure function of ``(seed, stream, m)``.
Row ``j`` of rank ``rank`` is global row ``g = rank·B + j`` (``g < 2³²``).  One
Philox4x32-10 call with counter ``(g, 0, stream, m mod 2³²)`` and key = (low,
high) words of the 64-bit seed gives words ``w0 … w3``;
``start = ((w1 << 32) | w0) mod (n − S)`` and the row is
``tokens[start : start + S + 1]``: ``idx`` its first ``S`` tokens, ``tgt`` its
last ``S``.  ``stream`` is 0 for training and 1 for evaluation.  The global
batch therefore depends on ``(seed, m)`` only — not on how ``world × B`` splits
it — and a checkpoint needs nothing but ``m``.  :func:`window_starts` is the
host reference of the kernel (``csrc/hip/data.hip``).

**Placement.**  On a GPU the corpus is device-resident when its ``2n`` bytes fit
``device_gb``: the kernel draws the starts and gathers in one launch, no host
round trip.  A larger corpus stays an ``np.memmap``: a background thread gathers
the next micro-batch's windows into one of two pinned ``[B, S + 1]`` buffers and
copies it on a side stream one micro-batch ahead; the compute stream waits on
the copy's event and the same kernel widens the staged buffer.  Both routes
produce identical ``idx`` / ``tgt``.  On the CPU the gather is numpy.

A token ``≥ vocab`` becomes ``idx 0`` / ``tgt −1`` (the embedding stays inside
its table, the cross-entropy skips the position) and is counted;
:meth:`TokenStream.check` raises with the file name and the count.  On a GPU
the count lives on the device and is read only where the trainer already
synchronises.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _native
from .ops.core import philox4x32_10

TRAIN_STREAM, EVAL_STREAM = 0, 1
_U32 = 0xFFFFFFFF


def window_starts(seed: int, stream: int, m: int, rank: int, B: int, n: int, S: int) -> np.ndarray:
    """Window starts of micro-batch ``m`` for rows ``rank·B … rank·B + B − 1`` of a
    corpus of ``n`` tokens: ``int64[B]``, each in ``[0, n − S − 1]`` (module docstring)."""
    if n < S + 1 or S < 1 or B < 1:
        raise ValueError(f"window_starts: need n >= S + 1, S >= 1 and B >= 1, got n={n}, S={S}, B={B}")
    if rank < 0 or (rank + 1) * B > 1 << 32:
        raise ValueError(f"window_starts: global rows rank*B + j must stay below 2^32 (rank={rank}, B={B})")
    g = np.arange(rank * B, (rank + 1) * B, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0, w1, _, _ = philox4x32_10((g, 0, int(stream), int(m) & _U32), (seed & _U32, seed >> 32))
    r = (w1 << np.uint64(32)) | w0
    return (r % np.uint64(n - S)).astype(np.int64)


def open_tokens(path: str, S: int, vocab: int) -> np.ndarray:
    """The token file as a read-only ``uint16`` memmap, after the format checks."""
    if vocab > 65536:
        raise ValueError(f"{path}: uint16 token files cannot feed a model of vocab_size {vocab} > 65536")
    size = os.path.getsize(path)
    if size % 2:
        raise ValueError(f"{path}: {size} bytes is not a whole number of uint16 tokens")
    if size // 2 < S + 1:
        raise ValueError(f"{path}: {size // 2} tokens, a window of seq {S} needs at least {S + 1}")
    return np.memmap(path, dtype="<u2", mode="r")


class TokenStream:
    """Micro-batches of one token file on one rank: ``batch(m) -> (idx, tgt)``,
    int64 ``[B, S]`` on ``device`` (module docstring)."""

    def __init__(self, path: str, B: int, S: int, vocab: int, device, seed: int = 0, stream: int = TRAIN_STREAM,
                 rank: int = 0, device_gb: float = 8.0):
        self.path, self.B, self.S, self.vocab = str(path), int(B), int(S), int(vocab)
        self.device = torch.device(device)
        self.seed, self.stream, self.rank = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(rank)
        if rank < 0 or (rank + 1) * B > 1 << 32:
            raise ValueError(f"global rows rank*B + j must stay below 2^32 (rank={rank}, B={B})")
        self.tokens = open_tokens(self.path, self.S, self.vocab)
        self.n = int(self.tokens.shape[0])
        self.bad_host = 0
        self.bad = self.corpus = None
        self._pool = None
        if self.device.type == "cuda":
            self._hip = _native.require_hip()
            self.bad = torch.zeros(1, dtype=torch.int64, device=self.device)
            if 2 * self.n <= device_gb * 2**30:
                # int16 carries the bits (the kernel reads them as uint16); uploaded in
                # 64 Mi-token pieces, so the host never holds a second copy of the file
                self.corpus = torch.empty(self.n, dtype=torch.int16, device=self.device)
                for o in range(0, self.n, 64 << 20):
                    piece = np.array(self.tokens[o:o + (64 << 20)]).view(np.int16)
                    self.corpus[o:o + piece.shape[0]].copy_(torch.from_numpy(piece))
            else:
                self._init_staging()
        self.placement = "cpu" if self.device.type != "cuda" else ("device" if self.corpus is not None else "host")

    # -- host side ----------------------------------------------------------
    def starts(self, m: int) -> np.ndarray:
        return window_starts(self.seed, self.stream, m, self.rank, self.B, self.n, self.S)

    def windows(self, m: int, out: np.ndarray | None = None) -> np.ndarray:
        """The ``[B, S + 1]`` uint16 windows of micro-batch ``m``, gathered on the host."""
        out = np.empty((self.B, self.S + 1), dtype=np.uint16) if out is None else out
        for r, s in enumerate(self.starts(m)):
            out[r] = self.tokens[s:s + self.S + 1]
        return out

    def host_batch(self, m: int):
        """``(idx, tgt, bad)`` of micro-batch ``m`` built with numpy: the reference of
        both GPU routes and the CPU trainer's path."""
        w = self.windows(m).astype(np.int64)
        ok = w < self.vocab
        idx = np.where(ok, w, 0)[:, :-1]
        tgt = np.where(ok, w, -1)[:, 1:]
        return (torch.from_numpy(np.ascontiguousarray(idx)), torch.from_numpy(np.ascontiguousarray(tgt)),
                int((~ok).sum()))

    # -- host-staged route --------------------------------------------------
    def _init_staging(self):
        import concurrent.futures as cf
        shape = (self.B, self.S + 1)
        self._pinned = [torch.empty(shape, dtype=torch.int16).pin_memory() for _ in range(2)]
        self._staged = [torch.empty(shape, dtype=torch.int16, device=self.device) for _ in range(2)]
        self._consumed = [None, None]  # compute-stream events: the kernel has read staged[k]
        self._side = torch.cuda.Stream(self.device)
        self._pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="pdo-data")
        self._next = None  # (m, future) of the micro-batch on its way
        self._slot = 0

    def _stage(self, m: int, k: int, consumed):
        """Worker thread: gather micro-batch ``m`` into pinned buffer ``k`` and copy it to
        staged buffer ``k`` on the side stream.  The pinned buffer is free (its previous
        copy was waited for below); the staged buffer is free once ``consumed``."""
        self.windows(m, self._pinned[k].numpy().view(np.uint16))
        with torch.cuda.stream(self._side):
            if consumed is not None:
                self._side.wait_event(consumed)
            self._staged[k].copy_(self._pinned[k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
        ev.synchronize()  # this thread only: the pinned buffer may be rewritten two micro-batches on
        return k, ev

    def _submit(self, m: int):
        k = self._slot
        self._slot ^= 1
        self._next = (m, self._pool.submit(self._stage, m, k, self._consumed[k]))

    def _staged_batch(self, m: int):
        if self._next is None or self._next[0] != m:
            if self._next is not None:
                self._next[1].result()  # a jump in m (resume, evaluation restart): drop what was on its way
            self._submit(m)
        k, ev = self._next[1].result()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        out = self._hip.token_batch(self._staged[k].view(-1), self.B * (self.S + 1), self.B, self.S, self.vocab, self.bad)
        done = torch.cuda.Event()
        done.record(cur)
        self._consumed[k] = done
        self._submit(m + 1)
        return out

    # -- API ------------------------------------------------------------------
    def batch(self, m: int):
        if self.corpus is not None:
            return self._hip.token_batch(self.corpus, self.n, self.B, self.S, self.vocab, self.bad,
                                         (self.seed, self.stream, int(m) & _U32, self.rank))
        if self._pool is not None:
            return self._staged_batch(m)
        idx, tgt, bad = self.host_batch(m)
        self.bad_host += bad
        self.check()  # no device to wait for: an out-of-range id stops the run before the model sees it
        return idx.to(self.device), tgt.to(self.device)

    def check(self):
        """Raise if any window token was ≥ vocab.  Reads the device counter (a sync)."""
        bad = self.bad_host + (int(self.bad.item()) if self.bad is not None else 0)
        if bad:
            raise ValueError(f"{self.path}: {bad} token id(s) >= vocab_size {self.vocab} in the sampled windows")

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
            self._next = None
