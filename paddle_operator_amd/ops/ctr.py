"""Sparse side of the CTR models (Wide&Deep, DeepFM): the fused lookup of a batch
and the deterministic sparse backward with row-wise Adagrad (``csrc/hip/ctr.hip``).

* ``ctr_lookup``       — one launch: gather the batch's deep rows next to its dense
  features (the tower's input ``X``), the wide sum and DeepFM's second-order term;
* ``ctr_sparse_step``  — segmented sum of the per-lookup gradients over the stably
  sorted ids, written as gradient rows (``GRAD``) or applied as ``ShardServer.push``'s
  Adagrad rule (``ADAGRAD``) to the rows the batch touched, in place;
* ``ref_ctr_lookup`` / ``ref_ctr_sparse_step`` — the same rules in plain torch, in the
  dtype of the tables they are given (fp32 or float64): the path of CPU tensors and of
  ``PDO_OPS=torch``, and the oracle of the tests.

Tables are ``deep [rows, D]`` and ``wide [rows]`` (or ``[rows, 1]``), ids are int64
``[B, S]``; an id outside ``[0, rows)`` reads zeros and contributes nothing.  The
device contract is ``D % 4 == 0`` and ``4 <= D <= 64``; both paths refuse anything else.
"""
from __future__ import annotations

import torch

from .. import _native
from .core import use_hip

GRAD, ADAGRAD = "grad", "adagrad"
_MODES = {GRAD: 0, ADAGRAD: 1}


def _check_dim(D: int):
    if D % 4 or not 4 <= D <= 64:
        raise ValueError(f"ctr: the embedding width must be a multiple of 4 in [4, 64], got {D}")


def min_ldx(S: int, D: int, n_dense: int) -> int:
    """Columns of ``X`` that hold values: the S gathered rows, then the dense features."""
    return S * D + n_dense


def padded_ldx(S: int, D: int, n_dense: int) -> int:
    """``min_ldx`` rounded up to 4 floats: rows of ``X`` and of ``dX`` then start on 16 B."""
    return (min_ldx(S, D, n_dense) + 3) // 4 * 4


def ref_ctr_lookup(ids, dense, deep, wide, fm: bool, ldx: int | None = None):
    """``(X, wide_sum, fm_term, ssum)`` in the tables' dtype; ``fm_term`` and ``ssum`` are
    ``None`` without ``fm``.  ``X [B, ldx]``: gathered rows, dense features, zeros."""
    B, S = ids.shape
    rows, D = deep.shape
    _check_dim(D)
    nd = dense.shape[1]
    K = min_ldx(S, D, nd)
    ldx = K if ldx is None else int(ldx)
    if ldx < K:
        raise ValueError(f"ctr: ldx {ldx} < S*D + n_dense = {K}")
    ok = (ids >= 0) & (ids < rows)
    safe = torch.where(ok, ids, torch.zeros_like(ids))
    e = torch.where(ok[..., None], deep[safe], deep.new_zeros(()))  # [B, S, D]; +0 outside the table
    w = torch.where(ok, wide.reshape(-1)[safe], wide.new_zeros(()))
    X = torch.zeros(B, ldx, dtype=deep.dtype, device=deep.device)
    X[:, :S * D] = e.reshape(B, S * D)
    X[:, S * D:K] = dense.to(deep.dtype)
    wide_sum = w.sum(dim=1)
    if not fm:
        return X, wide_sum, None, None
    ssum = e.sum(dim=1)
    fm_term = 0.5 * (ssum * ssum - (e * e).sum(dim=1)).sum(dim=1)
    return X, wide_sum, fm_term, ssum


def ref_run_sums(ids, dX, dlogit, ssum, deep):
    """The summed gradient of every id the batch holds: ``(uniq, g [U, D], g_w [U])``,
    per-lookup ``g = dX[b, slot·D : (slot+1)·D] + dlogit[b]·(ssum[b] − e)`` (the second
    term with ``ssum`` only), ``g_w = dlogit[b]``; ids outside the table are left out."""
    B, S = ids.shape
    rows, D = deep.shape
    dt = deep.dtype
    flat = ids.reshape(-1)
    ok = (flat >= 0) & (flat < rows)
    g = dX[:, :S * D].reshape(B * S, D).to(dt)
    dl = dlogit.to(dt).reshape(B, 1).expand(B, S).reshape(-1)
    if ssum is not None:
        safe = torch.where(ok, flat, torch.zeros_like(flat))
        ss = ssum.to(dt).reshape(B, 1, D).expand(B, S, D).reshape(B * S, D)
        g = g + dl[:, None] * (ss - deep[safe])
    uniq, inv = torch.unique(flat[ok], return_inverse=True)
    G = torch.zeros(uniq.numel(), D, dtype=dt, device=deep.device).index_add_(0, inv, g[ok])
    Gw = torch.zeros(uniq.numel(), dtype=dt, device=deep.device).index_add_(0, inv, dl[ok])
    return uniq, G, Gw


def ref_ctr_sparse_step(ids, dX, dlogit, ssum, tables, accs, lr, mode):
    """``ctr_sparse_step`` in plain torch, computed in the tables' dtype, in place."""
    deep, wide = tables
    o_deep, o_wide = accs
    _check_dim(deep.shape[1])
    if mode not in _MODES:
        raise ValueError(f"ctr: mode must be 'grad' or 'adagrad', not {mode!r}")
    uniq, G, Gw = ref_run_sums(ids, dX, dlogit, ssum, deep)
    wv, ov = wide.view(-1), o_wide.view(-1)
    if mode == GRAD:
        o_deep[uniq] = G
        ov[uniq] = Gw
        return
    lr = lr.to(deep.dtype).reshape(()) if torch.is_tensor(lr) else lr
    acc = o_deep[uniq] + G * G
    o_deep[uniq] = acc
    deep[uniq] = deep[uniq] - lr * G / acc.sqrt()
    accw = ov[uniq] + Gw * Gw
    ov[uniq] = accw
    wv[uniq] = wv[uniq] - lr * Gw / accw.sqrt()


def ctr_lookup(ids, dense, deep, wide, fm: bool, ldx: int | None = None):
    """``(X, wide_sum, fm_term, ssum)`` of a batch: ``X [B, ldx]`` holds the ``S`` gathered
    deep rows, then the dense features, then zeros (``ldx`` defaults to ``S·D + n_dense``);
    ``wide_sum [B]``; with ``fm`` the per-sample sum of the rows ``ssum [B, D]`` (kept
    for the backward) and DeepFM's second-order term ``fm_term [B]``, else ``None``."""
    if not use_hip(deep):
        return ref_ctr_lookup(ids, dense, deep, wide, fm, ldx)
    _check_dim(deep.shape[1])
    K = min_ldx(ids.shape[1], deep.shape[1], dense.shape[1])
    X, ws, fmt, ssum = _native.require_hip().ctr_fwd(ids.contiguous(), dense.contiguous(), deep, wide,
                                                     K if ldx is None else int(ldx), bool(fm))
    return (X, ws, fmt, ssum) if fm else (X, ws, None, None)


def ctr_sparse_step(ids, dX, dlogit, ssum, tables, accs, lr, mode):
    """The sparse backward of a batch, in place and deterministic.

    ``ids [B, S]``; ``dX [B, >= S·D]`` the gradient of ``ctr_lookup``'s ``X`` (rows may be
    strided); ``dlogit [B]``; ``ssum`` from ``ctr_lookup`` (``None``: no second-order
    term); ``tables = (deep, wide)``.  ``mode`` ``"grad"``: ``accs = (g_deep, g_wide)``
    receive the summed gradient of every id in the batch.  ``"adagrad"``: ``accs`` are the
    accumulators and the tables are updated, ``acc' = acc + g², w' = w − lr·g/√acc'``;
    ``lr`` is a float or a 1-element tensor on the tables' device (read at run time).
    Rows whose id is not in the batch are not touched."""
    deep, wide = tables
    if not use_hip(deep):
        return ref_ctr_sparse_step(ids, dX, dlogit, ssum, tables, accs, lr, mode)
    _check_dim(deep.shape[1])
    if mode not in _MODES:
        raise ValueError(f"ctr: mode must be 'grad' or 'adagrad', not {mode!r}")
    lr_dev = None
    if mode == ADAGRAD:
        lr_dev = lr if torch.is_tensor(lr) else torch.full((1,), float(lr), dtype=torch.float32, device=deep.device)
    keys, perm = torch.sort(ids.reshape(-1), stable=True)
    if dX.dim() != 2 or (dX.shape[1] > 1 and dX.stride(1) != 1):
        dX = dX.contiguous()
    _native.require_hip().ctr_bwd_rows(keys, perm, dX, dlogit.contiguous(), ssum, ids.shape[1], deep, wide, accs[0],
                                       accs[1], lr_dev, _MODES[mode])
