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

The ResNet trainer's image directories follow the same conventions:
:class:`ImageStream`, :func:`crop_boxes`, :func:`image_batch_ref` and ``IMAGE_DOC``
in the second part of this module (kernel ``csrc/hip/image.hip``), and so do the CTR
trainer's click directories: :class:`ClickStream`, :func:`record_index`, :func:`hash_rows`,
:func:`dense_norm`, :func:`click_batch_ref` and ``CLICK_DOC`` in the third part (kernel
``csrc/hip/click.hip``).
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


# ----------------------------------------------------------------------------------------------
# Image files and the replayable crop sampler of the ResNet trainer
# ----------------------------------------------------------------------------------------------
IMAGE_DOC = """
**File format.**  A directory with ``images.npy`` (uint8 ``[n, R, R, 3]``, RGB, square, C
order, ``R ≤ 4096``) and ``labels.npy`` (any integer dtype, ``[n]``, each in
``[0, classes)``), both opened with ``np.load(mmap_mode="r")``.  The model input is
``res × res`` with ``res % 8 == 0`` and ``8 ≤ res ≤ R``.

**Sampler.**  Counter-based like the token windows: the crops of micro-batch ``m`` are a pure
function of ``(seed, stream, m)``; row ``j`` of rank ``rank`` is global row ``g = rank·B + j``
(``g < 2³²``), key = (low, high) words of the 64-bit seed, and every value below is an unsigned
64-bit integer.  Training (stream 0) is a random-resized crop (area in [0.08, 1), aspect in
[3/4, 4/3]) and a flip:

* call A, counter ``(g, 0, stream, m)``: ``i = ((w1 << 32) | w0) mod n``, ``flip = w2 & 1``;
* call B, counter ``(g, 1, stream, m)`` → ``v0 … v3``:
  ``f = 5243 + (((v0 >> 16)·60293) >> 16)`` (area fraction, Q16),
  ``s = isqrt((f·R²) << 16)`` (side, Q16),
  ``t = 65536 + (((v1 >> 16)·10138) >> 16)`` (√ratio, Q16, in [1, √(4/3))),
  ``a = (s·t) >> 32``, ``b = ((s << 16) / t) >> 16``,
  ``(cw, ch) = (a, b) if v1 & 1 else (b, a)``, each clamped to ``[1, R]``,
  ``x0 = (v2·(R − cw + 1)) >> 32``, ``y0 = (v3·(R − ch + 1)) >> 32``.

Evaluation (stream 1) is not random: ``i = m·Bglobal + g`` (``Bglobal = world·B``), the centred
``res × res`` box (``x0 = y0 = (R − res) // 2``), no flip; a row with ``i ≥ n`` has label ``−1``
and a zero image (its box carries ``i = −1``), so ``ceil(n / Bglobal)`` micro-batches visit every
image exactly once for any ``world × B``.  :func:`crop_boxes` is the host reference of the draw.

**Resample.**  Signed Q16 source coordinates (x shown; y the same with ``ch``, ``y0``):
``step = (cw << 16) // res``; ``sx = ox·step + (step >> 1) − 32768`` clamped to
``[0, (cw − 1) << 16]``; ``ix = sx >> 16``, ``fx = (sx >> 8) & 255``, ``ix1 = min(ix + 1, cw − 1)``;
the source column is ``x0 + ix`` and a flipped row writes output column ``res − 1 − ox``.  The
four-tap sum ``Σ (256 − fy | fy)(256 − fx | fx)·p`` is an integer ``≤ 255·65536 < 2²⁴``, exact in
fp32, and the output is ``bf16_rne(fl(fl(float(sum)·sc[c]) + sh[c]))`` with
``sc = 1 / (65536·std)``, ``sh = −mean / std`` (``mean`` / ``std`` in pixel units: 255 × the
usual fractions, :func:`image_norm`).  At ``cw == res`` the fractions are zero: a copy.
The resample does not antialias: store the set at ``R ≈ 8/7·res``.  :func:`image_batch_ref` is
the host reference of the kernel (``csrc/hip/image.hip``) and the CPU trainer's path.

**Placement.**  As for tokens: device-resident when ``n·R²·3`` bytes fit ``device_gb`` (one
launch draws, resamples and stores); otherwise a worker gathers the next micro-batch's ``B``
stored images into one of two pinned buffers (≤ 4 threads) and copies it one micro-batch ahead
on a side stream, and the same kernel — still drawing geometry and flip itself — reads the
staged buffer.  Both routes write identical tensors.
"""

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GATHER_THREADS = 4  # a constant: a rank shares its node's CPUs with the other ranks


def image_norm(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """``(sc, sh)`` of the normalise step for per-channel ``mean`` / ``std`` of pixel / 255,
    rounded to fp32 as the kernel receives them (``sum`` carries a factor 65536)."""
    sc = tuple(float(np.float32(1.0 / (65536.0 * 255.0 * s))) for s in std)
    sh = tuple(float(np.float32(-m / s)) for m, s in zip(mean, std))
    return sc, sh


def crop_boxes(seed: int, stream: int, m: int, rank: int, B: int, n: int, R: int, res: int,
               Bglobal: int | None = None) -> np.ndarray:
    """The draw of micro-batch ``m`` for rows ``rank·B … rank·B + B − 1``: ``int64[B, 6]`` =
    ``i, x0, y0, cw, ch, flip`` (``IMAGE_DOC``; ``i = −1`` past the end of the evaluation set)."""
    import math
    if not (8 <= res <= R <= 4096 and res % 8 == 0 and n >= 1 and B >= 1):
        raise ValueError(f"crop_boxes: need 8 <= res <= R <= 4096, res % 8 == 0, n >= 1, B >= 1; got "
                         f"R={R}, res={res}, n={n}, B={B}")
    if rank < 0 or (rank + 1) * B > 1 << 32:
        raise ValueError(f"crop_boxes: global rows rank*B + j must stay below 2^32 (rank={rank}, B={B})")
    g = np.arange(rank * B, (rank + 1) * B, dtype=np.uint64)
    out = np.zeros((B, 6), dtype=np.int64)
    m32 = int(m) & _U32
    if stream != TRAIN_STREAM:
        Bglobal = B if Bglobal is None else int(Bglobal)
        base = m32 * Bglobal  # a Python int: up to 2^63
        if base < n:
            i = base + g.astype(np.int64)
            out[:, 0] = np.where(i < n, i, -1)
        else:
            out[:, 0] = -1
        out[:, 1] = out[:, 2] = (R - res) // 2
        out[:, 3] = out[:, 4] = res
        return out
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & _U32, seed >> 32)
    u = np.uint64
    w0, w1, w2, _ = philox4x32_10((g, 0, int(stream), m32), key)
    out[:, 0] = (((w1 << u(32)) | w0) % u(n)).astype(np.int64)
    out[:, 5] = (w2 & u(1)).astype(np.int64)
    v0, v1, v2, v3 = philox4x32_10((g, 1, int(stream), m32), key)
    f = u(5243) + (((v0 >> u(16)) * u(60293)) >> u(16))
    s = np.array([math.isqrt(int(x)) for x in (f * u(R * R)) << u(16)], dtype=np.uint64)
    t = u(65536) + (((v1 >> u(16)) * u(10138)) >> u(16))
    a, b = (s * t) >> u(32), ((s << u(16)) // t) >> u(16)
    odd = (v1 & u(1)) == u(1)
    cw = np.clip(np.where(odd, a, b).astype(np.int64), 1, R)
    ch = np.clip(np.where(odd, b, a).astype(np.int64), 1, R)
    out[:, 1] = ((v2 * (R - cw + 1).astype(np.uint64)) >> u(32)).astype(np.int64)
    out[:, 2] = ((v3 * (R - ch + 1).astype(np.uint64)) >> u(32)).astype(np.int64)
    out[:, 3], out[:, 4] = cw, ch
    return out


def _taps(c: int, res: int):
    """``(i0, i1, f)`` int64 arrays of one axis of the resample for a crop side ``c``."""
    step = (c << 16) // res
    s = np.clip(np.arange(res, dtype=np.int64) * step + (step >> 1) - 32768, 0, (c - 1) << 16)
    i0 = s >> 16
    return i0, np.minimum(i0 + 1, c - 1), (s >> 8) & 255


def bf16_rne_bits(x: np.ndarray) -> np.ndarray:
    """float32 array → the int16 bit patterns of its round-to-nearest-even bf16 values."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16).view(np.int16)


def image_batch_ref(images, labels, boxes: np.ndarray, res: int, sc, sh, staged: bool = False):
    """Host reference of ``image_batch``: ``(x, y)`` = bf16 ``[B, res, res, 3]`` and int64 ``[B]``
    torch tensors for the draw ``boxes`` (:func:`crop_boxes`).  ``staged``: row ``j`` reads
    ``images[j]`` / ``labels[j]``.  ``sc`` / ``sh``: three fp32 values each (``IMAGE_DOC``)."""
    B = boxes.shape[0]
    sc32, sh32 = np.asarray(sc, dtype=np.float32), np.asarray(sh, dtype=np.float32)
    x = np.zeros((B, res, res, 3), dtype=np.int16)
    y = np.full(B, -1, dtype=np.int64)
    for j, (i, x0, y0, cw, ch, flip) in enumerate(boxes.tolist()):
        if i < 0:
            continue
        src = j if staged else i
        y[j] = int(labels[src])
        iy0, iy1, fy = _taps(ch, res)
        ix0, ix1, fx = _taps(cw, res)
        im = np.asarray(images[src][y0:y0 + ch, x0:x0 + cw]).astype(np.int64)
        fy, fx = fy[:, None, None], fx[None, :, None]
        top, bot = im[iy0], im[iy1]
        tot = ((256 - fy) * ((256 - fx) * top[:, ix0] + fx * top[:, ix1])
               + fy * ((256 - fx) * bot[:, ix0] + fx * bot[:, ix1]))
        val = tot.astype(np.float32) * sc32 + sh32  # two fp32 roundings, as the kernel's multiply and add
        x[j] = bf16_rne_bits(val[:, ::-1] if flip else val)
    return torch.from_numpy(x).view(torch.bfloat16), torch.from_numpy(y)


def open_images(path: str, res: int, classes: int):
    """``(images, labels)`` memmaps of the directory ``path`` after the format checks."""
    fi, fl = os.path.join(path, "images.npy"), os.path.join(path, "labels.npy")
    images, labels = np.load(fi, mmap_mode="r"), np.load(fl, mmap_mode="r")
    if images.dtype != np.uint8:
        raise ValueError(f"{fi}: dtype {images.dtype}, images must be uint8")
    if images.ndim != 4 or images.shape[3] != 3 or images.shape[0] < 1:
        raise ValueError(f"{fi}: shape {images.shape}, images must be [n, R, R, 3] with n >= 1")
    if images.shape[1] != images.shape[2]:
        raise ValueError(f"{fi}: {images.shape[1]} x {images.shape[2]} images, they must be square")
    if not images.flags["C_CONTIGUOUS"]:
        raise ValueError(f"{fi}: images must be stored in C order")
    R = images.shape[1]
    if R > 4096 or R < res or res % 8 or res < 8:
        raise ValueError(f"{fi}: stored side R = {R} cannot feed a {res} x {res} input "
                         f"(8 <= res <= R <= 4096 and res % 8 == 0)")
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"{fl}: dtype {labels.dtype} shape {labels.shape}, labels must be integers [n]")
    if labels.shape[0] != images.shape[0]:
        raise ValueError(f"{fl}: {labels.shape[0]} labels for {images.shape[0]} images")
    lo, hi = int(labels.min()), int(labels.max())
    if lo < 0 or hi >= classes:
        raise ValueError(f"{fl}: labels span [{lo}, {hi}], outside [0, {classes})")
    return images, labels


class ImageStream:
    """Micro-batches of one image directory on one rank: ``batch(m, out=None) -> (x, y)``
    with ``x`` the ``[B, 3, res, res]`` input (bf16 channels_last on a GPU) and ``y`` int64
    ``[B]``; ``out = (xb, yb)`` are the caller's buffers (the captured step's inputs).
    """
    __doc__ += IMAGE_DOC

    def __init__(self, path: str, B: int, res: int, classes: int, device, seed: int = 0, stream: int = TRAIN_STREAM,
                 rank: int = 0, world: int = 1, device_gb: float = 8.0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.path, self.B, self.res, self.classes = str(path), int(B), int(res), int(classes)
        self.device = torch.device(device)
        self.seed, self.stream, self.rank = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(rank)
        self.Bglobal = int(world) * self.B
        if rank < 0 or rank >= world or self.Bglobal > 1 << 31:
            raise ValueError(f"need 0 <= rank < world and world*B <= 2^31 (rank={rank}, world={world}, B={B})")
        self.images, self.labels = open_images(self.path, self.res, self.classes)
        self.n, self.R = int(self.images.shape[0]), int(self.images.shape[1])
        self.norm = image_norm(mean, std)
        self.set = self.lab = None
        self._pool = None
        if self.device.type == "cuda":
            self._hip = _native.require_hip()
            if self.n * self.R * self.R * 3 <= device_gb * 2**30:
                # uploaded in pieces of about 256 MiB, so the host never holds a second copy of the file
                self.set = torch.empty((self.n, self.R, self.R, 3), dtype=torch.uint8, device=self.device)
                per = max(1, (256 << 20) // (self.R * self.R * 3))
                for o in range(0, self.n, per):
                    self.set[o:o + per].copy_(torch.from_numpy(np.array(self.images[o:o + per])))
                self.lab = torch.from_numpy(np.asarray(self.labels).astype(np.int32)).to(self.device)
            else:
                self._init_staging()
        self.placement = "cpu" if self.device.type != "cuda" else ("device" if self.set is not None else "host")

    def batches_per_epoch(self) -> int:
        """Micro-batches of the evaluation stream that cover the file once: ``ceil(n / (world·B))``."""
        return -(-self.n // self.Bglobal)

    # -- host side ----------------------------------------------------------
    def boxes(self, m: int) -> np.ndarray:
        return crop_boxes(self.seed, self.stream, m, self.rank, self.B, self.n, self.R, self.res, self.Bglobal)

    def host_batch(self, m: int):
        """``(x, y)`` of micro-batch ``m`` built with numpy (bf16 NHWC, int64): the reference of
        both GPU routes and the CPU trainer's path."""
        return image_batch_ref(self.images, self.labels, self.boxes(m), self.res, *self.norm)

    def _gather(self, idx, img_out: np.ndarray, lab_out: np.ndarray, pool=None):
        """Stored images ``idx`` (−1: past the end, left as they are) into ``img_out`` / ``lab_out``."""
        def part(rows):
            for r in rows:
                if idx[r] >= 0:
                    img_out[r] = self.images[idx[r]]
                    lab_out[r] = self.labels[idx[r]]
        chunks = [range(k, len(idx), GATHER_THREADS) for k in range(GATHER_THREADS)]
        if pool is None:
            part(range(len(idx)))
            return
        futs = [pool.submit(part, c) for c in chunks[1:]]
        part(chunks[0])
        for f in futs:
            f.result()

    # -- host-staged route --------------------------------------------------
    def _init_staging(self):
        import concurrent.futures as cf
        shape = (self.B, self.R, self.R, 3)
        self._pinned = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._pinned_lab = [torch.zeros(self.B, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._staged = [torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self._staged_lab = [torch.zeros(self.B, dtype=torch.int32, device=self.device) for _ in range(2)]
        self._consumed = [None, None]  # compute-stream events: the kernel has read staged[k]
        self._side = torch.cuda.Stream(self.device)
        # one staging task at a time; it gathers a share itself and hands the rest to the other workers
        self._pool = cf.ThreadPoolExecutor(max_workers=GATHER_THREADS, thread_name_prefix="pdo-data")
        self._next = None  # (m, future) of the micro-batch on its way
        self._slot = 0

    def _stage(self, m: int, k: int, consumed):
        """Worker thread: gather micro-batch ``m`` into pinned buffers ``k`` and copy them to the
        staged buffers ``k`` on the side stream (the event discipline of ``TokenStream._stage``)."""
        self._gather(self.boxes(m)[:, 0], self._pinned[k].numpy(), self._pinned_lab[k].numpy(), self._pool)
        with torch.cuda.stream(self._side):
            if consumed is not None:
                self._side.wait_event(consumed)
            self._staged[k].copy_(self._pinned[k], non_blocking=True)
            self._staged_lab[k].copy_(self._pinned_lab[k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
        ev.synchronize()  # this thread only: the pinned buffers may be rewritten two micro-batches on
        return k, ev

    def _submit(self, m: int):
        k = self._slot
        self._slot ^= 1
        self._next = (m, self._pool.submit(self._stage, m, k, self._consumed[k]))

    def _staged_batch(self, m: int, xb, yb):
        if self._next is None or self._next[0] != m:
            if self._next is not None:
                self._next[1].result()  # a jump in m (resume, evaluation restart): drop what was on its way
            self._submit(m)
        k, ev = self._next[1].result()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        out = self._launch(self._staged[k], self._staged_lab[k], m, True, xb, yb)
        done = torch.cuda.Event()
        done.record(cur)
        self._consumed[k] = done
        self._submit(m + 1)
        return out

    def _launch(self, img, lab, m, staged, xb, yb):
        return self._hip.image_batch(img, lab, self.n, self.B, self.R, self.res, self.norm,
                                     (self.seed, self.stream, int(m) & _U32, self.rank), self.Bglobal, staged, xb, yb)

    # -- API ------------------------------------------------------------------
    def batch(self, m: int, out=None):
        xb, yb = out if out is not None else (None, None)
        direct = (xb is None or (xb.is_cuda and xb.dtype == torch.bfloat16 and xb.is_contiguous()
                                 and tuple(xb.shape) == (self.B, self.res, self.res, 3)))
        if self.device.type == "cuda":
            tx = xb if direct else None
            x, y = (self._launch(self.set, self.lab, m, False, tx, yb) if self.set is not None
                    else self._staged_batch(m, tx, yb))
        else:
            x, y = self.host_batch(m)
            if yb is not None:
                yb.copy_(y)
                y = yb
        x = x.permute(0, 3, 1, 2)  # NHWC memory: a channels_last [B, 3, res, res]
        if xb is not None and not direct:  # an NCHW / fp32 buffer (the CPU trainer): one converting copy
            xb.copy_(x)
            x = xb
        return x, y

    def close(self):
        if self._pool is not None:
            if self._next is not None:
                self._next[1].result()
            self._pool.shutdown(wait=True)
            self._pool = None
            self._next = None


# ----------------------------------------------------------------------------------------------
# Click logs and the replayable record sampler of the CTR trainer (Wide&Deep, DeepFM)
# ----------------------------------------------------------------------------------------------
CLICK_DOC = """
**File format.**  A directory of four arrays opened with ``np.load(mmap_mode="r")``, all in C
order, ``1 ≤ n < 2³¹`` records: ``cat.npy`` (uint32 ``[n, S]``, the raw categorical value of
each slot — Criteo's 8-hex-digit tokens are exactly 32 bits; ``0`` is the value written for a
missing field and is hashed like any other), ``dense.npy`` (int32 ``[n, n_dense]``, the raw
integer features, ``−2³¹`` = missing), ``label.npy`` (uint8 ``[n]``, 0 or 1) and
``dense_stats.npy`` (float32 ``[2, n_dense]``: row 0 ``min``, row 1 ``diff``; all finite,
``diff > 0``).  ``S`` and ``n_dense`` are the model's ``n_sparse`` / ``n_dense``.

**Draw.**  The image sampler's convention: row ``j`` of rank ``rank`` is global row
``g = rank·B + j`` (``g < 2³²``), key = (low, high) words of the 64-bit seed.  Training
(stream 0): one Philox4x32-10 call with counter ``(g, 0, stream, m mod 2³²)``,
``i = ((w1 << 32) | w0) mod n`` — sampling with replacement.  Evaluation (stream 1) is not
random: ``i = (m mod 2³²)·Bglobal + g`` (``Bglobal = world·B``); a row with ``i ≥ n`` is a pad
row — every id ``−1``, every dense value ``+0.0``, label ``−1`` — so ``ceil(n / Bglobal)``
batches visit every record exactly once for any ``world × B``.  :func:`record_index` is the
host reference of the draw (``−1`` on a pad row).

**Hash.**  Slot ``s``, raw value ``c``, ``V = vocab_per_slot ∈ [1, 2³¹]``:
``salt_s = ((s + 1)·0x9E3779B9) mod 2³²``; ``h = fmix32(c ^ salt_s)``, murmur3's finaliser
(``h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16``, all mod 2³²);
``ids[j, s] = s·V + ((h·V) >> 32)`` in 64-bit arithmetic.  ``fmix32`` is a bijection, so distinct
values of one slot collide only through the reduction to ``V``.  :func:`hash_rows`.

**Dense.**  ``dense[j, k] = +0.0`` if the stored value is ``−2³¹``, otherwise
``fl(fl(float(v) − min[k]) / diff[k])``: ``float(v)`` is the round-to-nearest-even int → fp32
conversion and the division the correctly rounded IEEE one — the min–max rule of Paddle's
Criteo readers, exact in numpy float32.  :func:`dense_norm`.

**Label.**  ``float(label[i])``.

**Outputs.**  ``ids`` int64 ``[B, S]``, ``dense`` fp32 ``[B, n_dense]``, ``label`` fp32 ``[B]``:
what ``ops.ctr_lookup`` and the loss take.  ``ctr_lookup`` reads zeros for id ``−1`` and the
sparse step ignores it.  :func:`click_batch_ref` is the host reference of the kernel
(``csrc/hip/click.hip``) and the CPU trainer's path.

**Placement.**  As for tokens and images: device-resident when ``n·(4S + 4n_dense + 1)`` bytes
fit ``device_gb`` (one launch draws, hashes, normalises and stores); otherwise a worker gathers
the next batch's ``B`` records into one of two pinned buffer sets and copies them one batch ahead
on a side stream, and the same kernel — still drawing the record, so that it knows the pad
rows — reads the staged buffers.  Both routes write identical tensors.
"""

_I32_MIN = -(1 << 31)


def record_index(seed: int, stream: int, m: int, rank: int, B: int, n: int, Bglobal: int | None = None) -> np.ndarray:
    """The records of batch ``m`` for rows ``rank·B … rank·B + B − 1``: ``int64[B]``, ``−1`` past
    the end of the evaluation set (``CLICK_DOC``)."""
    if not (1 <= n < 1 << 31 and B >= 1):
        raise ValueError(f"record_index: need 1 <= n < 2^31 and B >= 1, got n={n}, B={B}")
    if rank < 0 or (rank + 1) * B > 1 << 32:
        raise ValueError(f"record_index: global rows rank*B + j must stay below 2^32 (rank={rank}, B={B})")
    g = np.arange(rank * B, (rank + 1) * B, dtype=np.uint64)
    m32 = int(m) & _U32
    if stream != TRAIN_STREAM:
        base = m32 * (B if Bglobal is None else int(Bglobal))  # a Python int: up to 2^63
        if base >= n:
            return np.full(B, -1, dtype=np.int64)
        i = base + g.astype(np.int64)
        return np.where(i < n, i, -1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0, w1, _, _ = philox4x32_10((g, 0, int(stream), m32), (seed & _U32, seed >> 32))
    return (((w1 << np.uint64(32)) | w0) % np.uint64(n)).astype(np.int64)


def hash_rows(cat: np.ndarray, V: int) -> np.ndarray:
    """Table rows of the raw values ``cat`` (uint32 ``[..., S]``, slot = last axis): int64 of the
    same shape, ``s·V + ((fmix32(c ^ salt_s)·V) >> 32)`` (``CLICK_DOC``)."""
    if not 1 <= V <= 1 << 31:
        raise ValueError(f"hash_rows: vocab_per_slot must be in [1, 2^31], got {V}")
    u, mask = np.uint64, np.uint64(_U32)
    s = np.arange(cat.shape[-1], dtype=np.uint64)
    h = (np.asarray(cat).astype(np.uint64) ^ (((s + u(1)) * u(0x9E3779B9)) & mask))
    h ^= h >> u(16)
    h = (h * u(0x85EBCA6B)) & mask
    h ^= h >> u(13)
    h = (h * u(0xC2B2AE35)) & mask
    h ^= h >> u(16)
    return (s * u(V) + ((h * u(V)) >> u(32))).astype(np.int64)


def dense_norm(raw: np.ndarray, stats: np.ndarray) -> np.ndarray:
    """``(float(v) − min) / diff`` in float32, ``+0.0`` where the stored value is ``−2³¹``
    (``raw`` int32 ``[..., n_dense]``, ``stats`` float32 ``[2, n_dense]``; ``CLICK_DOC``)."""
    raw = np.asarray(raw, dtype=np.int32)
    stats = np.asarray(stats, dtype=np.float32)
    x = (raw.astype(np.float32) - stats[0]) / stats[1]  # each operation rounds once, to nearest even
    return np.where(raw == _I32_MIN, np.float32(0.0), x).astype(np.float32)


def click_batch_ref(cat, dense, label, stats, rec: np.ndarray, V: int, staged: bool = False):
    """Host reference of ``click_batch``: ``(ids, dense, label)`` = int64 ``[B, S]``, fp32
    ``[B, n_dense]`` and fp32 ``[B]`` torch tensors for the drawn records ``rec``
    (:func:`record_index`).  ``staged``: row ``j`` reads entry ``j`` of the arrays."""
    rec = np.asarray(rec, dtype=np.int64)
    B, live = rec.shape[0], rec >= 0
    src = np.flatnonzero(live) if staged else rec[live]
    ids = np.full((B, cat.shape[1]), -1, dtype=np.int64)
    x = np.zeros((B, dense.shape[1]), dtype=np.float32)
    y = np.full(B, -1.0, dtype=np.float32)
    if src.size:
        ids[live] = hash_rows(np.asarray(cat)[src], V)
        x[live] = dense_norm(np.asarray(dense)[src], stats)
        y[live] = np.asarray(label)[src].astype(np.float32)
    return torch.from_numpy(ids), torch.from_numpy(x), torch.from_numpy(y)


def open_clicks(path: str, S: int, n_dense: int):
    """``(cat, dense, label, stats)`` of the click directory ``path`` after the format checks
    (the first three are memmaps, ``stats`` a float32 array)."""
    fc, fd, fl, fs = (os.path.join(path, f) for f in ("cat.npy", "dense.npy", "label.npy", "dense_stats.npy"))
    cat, dense, label = (np.load(f, mmap_mode="r") for f in (fc, fd, fl))
    stats = np.load(fs, mmap_mode="r")
    for f, a, dt in ((fc, cat, np.uint32), (fd, dense, np.int32), (fl, label, np.uint8), (fs, stats, np.float32)):
        if a.dtype != dt:
            raise ValueError(f"{f}: dtype {a.dtype}, must be {np.dtype(dt)}")
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{f}: must be stored in C order")
    if cat.ndim != 2 or cat.shape[1] != S:
        raise ValueError(f"{fc}: shape {cat.shape}, the model has {S} sparse slots: [n, {S}] expected")
    n = cat.shape[0]
    if not 1 <= n < 1 << 31:
        raise ValueError(f"{fc}: {n} records, 1 <= n < 2^31 required")
    if dense.ndim != 2 or dense.shape[1] != n_dense:
        raise ValueError(f"{fd}: shape {dense.shape}, the model has {n_dense} dense features: [n, {n_dense}] expected")
    if dense.shape[0] != n:
        raise ValueError(f"{fd}: {dense.shape[0]} records, {fc} has {n}")
    if label.ndim != 1 or label.shape[0] != n:
        raise ValueError(f"{fl}: shape {label.shape}, {fc} has {n} records: [{n}] expected")
    if int(label.max()) > 1:
        raise ValueError(f"{fl}: labels must be 0 or 1, found {int(label.max())}")
    return cat, dense, label, check_click_stats(stats, n_dense, fs)


def check_click_stats(stats, n_dense: int, name: str) -> np.ndarray:
    """``stats`` as a float32 ``[2, n_dense]`` array (min, diff) after its checks."""
    stats = np.array(stats)
    if stats.dtype != np.float32 or stats.shape != (2, n_dense):
        raise ValueError(f"{name}: dtype {stats.dtype} shape {stats.shape}, must be float32 [2, {n_dense}]")
    if not np.isfinite(stats).all() or not (stats[1] > 0).all():
        raise ValueError(f"{name}: min and diff must be finite and diff > 0")
    return stats


class ClickStream:
    """Batches of one click directory on one rank: ``batch(m) -> (ids, dense, label)``, int64
    ``[B, S]``, fp32 ``[B, n_dense]`` and fp32 ``[B]`` on ``device``.  ``stats`` (float32
    ``[2, n_dense]``) replaces the directory's own ``dense_stats.npy``: a validation stream is
    normalised with the training set's.
    """
    __doc__ += CLICK_DOC

    def __init__(self, path: str, B: int, S: int, n_dense: int, vocab_per_slot: int, device, seed: int = 0,
                 stream: int = TRAIN_STREAM, rank: int = 0, world: int = 1, device_gb: float = 8.0, stats=None):
        self.path, self.B, self.S, self.n_dense, self.V = str(path), int(B), int(S), int(n_dense), int(vocab_per_slot)
        self.device = torch.device(device)
        self.seed, self.stream, self.rank = int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(rank)
        self.Bglobal = int(world) * self.B
        if rank < 0 or rank >= world or self.Bglobal > 1 << 31:
            raise ValueError(f"need 0 <= rank < world and world*B <= 2^31 (rank={rank}, world={world}, B={B})")
        if not 1 <= self.V <= 1 << 31:
            raise ValueError(f"vocab_per_slot must be in [1, 2^31], got {vocab_per_slot}")
        if self.B * self.S >= 1 << 31:
            raise ValueError(f"B*S must stay below 2^31 (B={B}, S={S})")
        self.cat, self.dense, self.label, own = open_clicks(self.path, self.S, self.n_dense)
        self.stats = own if stats is None else check_click_stats(stats, self.n_dense, "stats")
        self.n = int(self.cat.shape[0])
        self.set = None
        self._pool = None
        if self.device.type == "cuda":
            self._hip = _native.require_hip()
            self._stats_dev = torch.from_numpy(self.stats).to(self.device)
            if self.n * (4 * self.S + 4 * self.n_dense + 1) <= device_gb * 2**30:
                # uploaded in pieces of about 256 MiB, so the host never holds a second copy of the files;
                # int32 carries cat's bits (the kernel reads them as uint32)
                dev = self.device
                self.set = (torch.empty((self.n, self.S), dtype=torch.int32, device=dev),
                            torch.empty((self.n, self.n_dense), dtype=torch.int32, device=dev),
                            torch.empty(self.n, dtype=torch.uint8, device=dev))
                per = max(1, (256 << 20) // (4 * max(self.S, self.n_dense)))
                for o in range(0, self.n, per):
                    self.set[0][o:o + per].copy_(torch.from_numpy(np.array(self.cat[o:o + per]).view(np.int32)))
                    self.set[1][o:o + per].copy_(torch.from_numpy(np.array(self.dense[o:o + per])))
                    self.set[2][o:o + per].copy_(torch.from_numpy(np.array(self.label[o:o + per])))
            else:
                self._init_staging()
        self.placement = "cpu" if self.device.type != "cuda" else ("device" if self.set is not None else "host")

    def batches_per_epoch(self) -> int:
        """Batches of the evaluation stream that cover the set once: ``ceil(n / (world·B))``."""
        return -(-self.n // self.Bglobal)

    # -- host side ----------------------------------------------------------
    def records(self, m: int) -> np.ndarray:
        return record_index(self.seed, self.stream, m, self.rank, self.B, self.n, self.Bglobal)

    def host_batch(self, m: int):
        """``(ids, dense, label)`` of batch ``m`` built with numpy: the reference of both GPU
        routes and the CPU trainer's path."""
        return click_batch_ref(self.cat, self.dense, self.label, self.stats, self.records(m), self.V)

    def _gather(self, m: int, outs):
        """The records of batch ``m`` into the ``[B, …]`` buffers ``outs`` = (cat, dense, label); a pad
        row's entry is left as it is."""
        rec = self.records(m)
        live = rec >= 0
        for a, o in zip((self.cat, self.dense, self.label), outs):
            if live.all():
                np.take(a, rec, axis=0, out=o, mode="clip")  # rec < n: nothing is clipped, no bounce buffer
            elif live.any():
                o[live] = a[rec[live]]

    # -- host-staged route --------------------------------------------------
    def _init_staging(self):
        import concurrent.futures as cf
        shapes = (((self.B, self.S), torch.int32), ((self.B, self.n_dense), torch.int32), ((self.B,), torch.uint8))
        self._pinned = [[torch.zeros(s, dtype=d).pin_memory() for s, d in shapes] for _ in range(2)]
        self._staged = [[torch.zeros(s, dtype=d, device=self.device) for s, d in shapes] for _ in range(2)]
        self._consumed = [None, None]  # compute-stream events: the kernel has read staged[k]
        self._side = torch.cuda.Stream(self.device)
        self._pool = cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="pdo-data")
        self._next = None  # (m, future) of the batch on its way
        self._slot = 0

    def _stage(self, m: int, k: int, consumed):
        """Worker thread: gather batch ``m`` into the pinned buffers ``k`` and copy them to the
        staged buffers ``k`` on the side stream (the event discipline of ``ImageStream._stage``)."""
        pc, pd, pl = self._pinned[k]
        self._gather(m, (pc.numpy().view(np.uint32), pd.numpy(), pl.numpy()))
        with torch.cuda.stream(self._side):
            if consumed is not None:
                self._side.wait_event(consumed)
            for dst, src in zip(self._staged[k], self._pinned[k]):
                dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._side)
        ev.synchronize()  # this thread only: the pinned buffers may be rewritten two batches on
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
        out = self._launch(self._staged[k], m, True)
        done = torch.cuda.Event()
        done.record(cur)
        self._consumed[k] = done
        self._submit(m + 1)
        return out

    def _launch(self, arrays, m, staged):
        cat, dense, label = arrays
        return self._hip.click_batch(cat, dense, label, self._stats_dev, self.n, self.B, self.S, self.n_dense, self.V,
                                     (self.seed, self.stream, int(m) & _U32, self.rank), self.Bglobal, staged)

    # -- API ------------------------------------------------------------------
    def batch(self, m: int):
        if self.set is not None:
            return self._launch(self.set, m, False)
        if self._pool is not None:
            return self._staged_batch(m)
        return tuple(t.to(self.device) for t in self.host_batch(m))

    def close(self):
        if self._pool is not None:
            if self._next is not None:
                self._next[1].result()
            self._pool.shutdown(wait=True)
            self._pool = None
            self._next = None
