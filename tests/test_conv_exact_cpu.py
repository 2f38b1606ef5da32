"""CPU self-checks of what test_conv_exact_gpu.py and test_gemm_dw_exact_gpu.py hold the kernels to:
the float64 references against independent formulations, the exactness preconditions of every table
entry, the dispatch each weight-gradient shape is listed for, and the comparison helpers on mutated
references (they must fail, and name the right coordinate)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_conv_exact_gpu as cg
import test_gemm_dw_exact_gpu as gg
from test_conv_exact_gpu import (ALL_PATHS, KRSC, NEEDLE_SHAPES, NHWC, SHAPES, STEM_SHAPES, WGRAD, WGRAD_MODES, case,
                                 check_bits, conv_ref, exact_bound, first_mismatch, fold_template, geometry,
                                 grads_ref, needle_dgrad_ref, needle_fwd_ref, needle_input, needle_weight, nhwc,
                                 rne_bf16, s2d_ref, sid, stem_case, stride2_add_ref, tile_stats_ref, wgrad_plan)

F64 = torch.float64
BF16 = torch.bfloat16
SMALL = SHAPES[:4]  # the table's smallest shapes: 3x3 stride 1 at both tile widths, 3x3 stride 2


def unfold_conv(x, w, stride):
    """The convolution as im2col + matmul."""
    N, C, H, W = x.shape
    K, _, R, _ = w.shape
    pad = (R - 1) // 2
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    cols = F.unfold(x, R, padding=pad, stride=stride)  # [N, C*R*R, Ho*Wo]
    return (w.reshape(K, -1) @ cols).reshape(N, K, Ho, Wo)


@pytest.mark.parametrize("shape", SMALL, ids=sid)
def test_references_match_independent_formulations(shape):
    """conv_ref against F.unfold + matmul; grads_ref against autograd through that formulation
    (integers: every formulation gives the same float64 value exactly)."""
    c = case(shape)
    st = shape[6]
    assert torch.equal(c["y"], unfold_conv(c["x"], c["w"], st))
    xr, wr = c["x"].clone().requires_grad_(), c["w"].clone().requires_grad_()
    dx, dw = torch.autograd.grad(unfold_conv(xr, wr, st), (xr, wr), c["dy"])
    assert torch.equal(c["dx"], dx) and torch.equal(c["dw"], dw)
    gx, gw = grads_ref(c["x"], c["w"], c["dy"], st)
    assert torch.equal(gx, dx) and torch.equal(gw, dw)


@pytest.mark.parametrize("N,H,W", STEM_SHAPES)
def test_stem_references(N, H, W):
    """s2d_ref against pixel_unshuffle (its channel order is c*4 + 2p + q); the stem convolution
    against unfold + matmul and as the 4x4 stride-1 convolution over z the kernels run."""
    c = stem_case(N, H, W)
    pu = F.pixel_unshuffle(c["x"], 2).reshape(N, 3, 4, H // 2, W // 2)  # [n][c][2p + q][i][j]
    want = torch.zeros_like(c["z"])
    want[:, :12] = pu.permute(0, 2, 1, 3, 4).reshape(N, 12, H // 2, W // 2)
    assert torch.equal(c["z"], want)
    cols = F.unfold(c["x"], 7, padding=3, stride=2)
    assert torch.equal(c["y"], (c["w"].reshape(64, -1) @ cols).reshape(c["y"].shape))
    # w8[r + 1][s + 1] = w[r][s]; w2[k][(2p + q)*3 + c][a][b] = w8[k][c][2a + p][2b + q]: y = conv4x4(z, w2),
    # pad 2 before / 1 after
    w8 = F.pad(c["w"], (1, 0, 1, 0))
    w2 = torch.zeros(64, 16, 4, 4, dtype=F64)
    for p in range(2):
        for q in range(2):
            w2[:, (2 * p + q) * 3:(2 * p + q) * 3 + 3] = w8[:, :, p::2, q::2]
    assert torch.equal(c["y"], F.conv2d(F.pad(c["z"], (2, 1, 2, 1)), w2))


def test_preconditions_hold_for_every_table_entry():
    """The < 2^24 bound of every convolution case (case() asserts it while building), input ranges,
    and the shapes' geometry: non-square or odd where the table says so."""
    for shape in sorted(set(SHAPES) | {s for s, _, _ in WGRAD} | {ALL_PATHS} | set(NEEDLE_SHAPES)):
        N, C, H, W, K, R, st = shape
        pad, Ho, Wo, M = geometry(shape)
        c = case(shape)
        assert exact_bound(R * R * C, cg.X_MAX, cg.W_MAX) < cg.LIM
        assert exact_bound(M, cg.DY_MAX, cg.X_MAX, cg.ADD_MAX) < cg.LIM
        for name in ("y", "dx", "dw"):
            assert bool((c[name] == c[name].round()).all()) and float(c[name].abs().max()) < cg.LIM
        # most outputs are bf16-exact (|v| <= 256) except at the longest reduction
        if R * R * C <= 1152:
            assert float((c["y"].abs() <= 256).double().mean()) > 0.99, sid(shape)
    assert all(H != W for _, _, H, W, _, _, _ in SHAPES if (H, W) != (7, 7))
    assert {geometry(s)[3] for s in SHAPES} >= {12, 45, 147, 4480}


def test_wgrad_table_reaches_every_path_and_fold():
    """Every weight-gradient shape dispatches to the path it is listed for, and together the table
    reaches the four per-tap templates, both tap-group widths, the gathered path's special cases and
    all three fold templates."""
    plans = []
    for shape, path, why in WGRAD:
        plan = wgrad_plan(shape, *WGRAD_MODES[path])
        assert plan["path"] == path, (shape, why, plan)
        plans.append((shape, plan))
    assert {(p["bm"], p["bn"]) for _, p in plans if p["path"] == "pertap"} == {(64, 64), (128, 64), (64, 128), (128, 128)}
    assert {s[1] for s, p in plans if p["path"] == "taps"} == {64, 128}
    assert {p["fold"] for _, p in plans} == {1, 4, 16}
    assert any(p["path"] == "taps" and p["splits"] >= 16 for _, p in plans)
    assert any(p["path"] == "taps" and geometry(s)[3] % 64 for s, p in plans)
    assert any(p["path"] == "taps" and s[6] == 2 for s, p in plans)
    gather = [(s, p) for s, p in plans if p["path"] == "gather"]
    assert any(geometry(s)[3] == 256 and p["splits"] == 1 for s, p in gather)
    assert any(s[4] == 128 for s, _ in gather) and any(s[5] ** 2 * s[1] == 1152 and s[4] == 256 for s, _ in gather)
    assert any(s[6] == 2 for s, _ in gather) and any(p["splits"] >= 2 for _, p in gather)
    assert {wgrad_plan(ALL_PATHS, *WGRAD_MODES[p])["path"] for p in WGRAD_MODES} == {"taps", "gather", "pertap"}
    assert fold_template(16, 64, 576) == 16 and fold_template(16, 256, 2304) == 4 and fold_template(3, 64, 64) == 1


@pytest.mark.parametrize("shape", NEEDLE_SHAPES, ids=sid)
def test_needle_references_match_conv(shape):
    N, C, H, W, K, R, st = shape
    pad, Ho, Wo, _ = geometry(shape)
    w = needle_weight(K, C, R)
    assert len({float(v) for v in w[0, 0].reshape(-1)}) == R * R  # distinct per tap
    y, taps = needle_fwd_ref(shape, 37)
    assert torch.equal(y, conv_ref(needle_input(N, C, H, W, 37), w, st))
    assert set(taps) == {tuple(i) for i in nhwc(y).abs().sum(-1).nonzero().tolist()}
    dx, taps = needle_dgrad_ref(shape, 37)
    dy = needle_input(N, K, Ho, Wo, 37)
    assert torch.equal(dx, grads_ref(torch.zeros(N, C, H, W, dtype=F64), w, dy, st)[0])
    assert set(taps) == {tuple(i) for i in nhwc(dx).abs().sum(-1).nonzero().tolist()}


def test_stride2_add_reference_rounds_once():
    dx = torch.tensor([[[[257.0, -0.5], [-1.5, -2.5]]]], dtype=F64)
    add = torch.tensor([[[[2.0]]]], dtype=F64)
    out = stride2_add_ref(dx, add)
    assert out.dtype == BF16 and out.flatten().tolist() == [260.0, -0.5, -1.5, -2.5]  # 259 ties to even 260


# ---------------------------------------------------------------------------------------------
# the comparison helpers on mutated references
# ---------------------------------------------------------------------------------------------
def test_mismatch_names_a_dropped_token():
    shape = SHAPES[1]  # 1 x 64 x 5 x 9
    c = case(shape)
    want = rne_bf16(c["y"])
    assert first_mismatch(nhwc(want.clone()), nhwc(want), NHWC) is None
    got = want.clone()
    got[0, :, 3, 7] = 0  # token (0, 3, 7) never stored
    k = int((want[0, :, 3, 7] != 0).nonzero()[0])
    msg = first_mismatch(nhwc(got), nhwc(want), NHWC)
    assert msg.startswith(f"first mismatch at n 0, h 3, w 7, channel {k}:"), msg
    with pytest.raises(AssertionError, match="n 0, h 3, w 7"):
        check_bits(nhwc(got), nhwc(want), NHWC, "dropped token")
    # a token dropped from the weight gradient's reduction changes dw wherever dy[t] x[pixel] != 0
    dy = c["dy"].clone()
    dy[0, :, 3, 7] = 0
    dw = grads_ref(c["x"], c["w"], dy, shape[6])[1]
    diff = (nhwc(dw) != nhwc(c["dw"])).reshape(-1).nonzero()[0]
    msg = first_mismatch(nhwc(cg.exact_f32(dw)), nhwc(cg.exact_f32(c["dw"])), KRSC)
    idx = []
    flat = int(diff)
    for d in reversed(nhwc(dw).shape):
        idx.append(flat % d)
        flat //= d
    k, r, s, ci = reversed(idx)
    assert msg.startswith(f"first mismatch at kout {k}, r {r}, s {s}, cin {ci}:"), msg


def test_mismatch_names_a_tap_read_across_the_padding_edge():
    """Tap (r = 1, s = 0) of output pixel (1, 0) must read padding; a kernel without the column check
    reads the previous row's last pixel instead.  The helper names that output pixel."""
    shape = SHAPES[1]
    N, C, H, W, K, R, st = shape
    c = case(shape)
    y = c["y"].clone()
    y[0, :, 1, 0] += c["w"][:, :, 1, 0] @ c["x"][0, :, 0, W - 1]
    k = int((y[0, :, 1, 0] != c["y"][0, :, 1, 0]).nonzero()[0])
    msg = first_mismatch(nhwc(y.float()), nhwc(c["y"].float()), NHWC)
    assert msg.startswith(f"first mismatch at n 0, h 1, w 0, channel {k}:"), msg


def test_tile_statistics_notice_a_row_past_the_last_token():
    """The last partial tile's statistics over one row too many differ from tile_stats_ref's, at that
    tile; full tiles are unchanged."""
    torch.manual_seed(0)
    M, K, tile = 147, 8, 128
    rows = torch.randint(-50, 51, (M + 1, K)).to(F64)
    rows[M] = 7.0  # what a kernel would read past the last token
    ref = tile_stats_ref(rows[:M], tile)
    assert ref.shape == (2, 2, K)
    assert torch.equal(ref[1, 0], rows[128:147].sum(0))
    assert torch.allclose(ref[1, 1], rows[128:147].var(0, unbiased=False) * 19, rtol=1e-12)
    leak = tile_stats_ref(rows, tile)
    assert torch.equal(leak[0], ref[0])
    msg = first_mismatch(leak[:, 0].float(), ref[:, 0].float(), ("tile", "channel"))
    assert msg.startswith("first mismatch at tile 1, channel 0:"), msg


@pytest.mark.parametrize("d", [3, 5, 6, 7, 9, 12, 40, 56, 112, 1023, 4097])
def test_float_reciprocal_divmod_is_exact_below_2_24(d):
    """The kernels split a token index with q = int(float(x) * (1.f / d)) and one correction step
    (conv.hip divmod).  The same float32 arithmetic here: exact for the table's extents and a few
    others, at every x of the top 2^18 below 2^24 (conv_supported's token limit) and every 61st below."""
    inv = np.float32(1.0) / np.float32(d)
    x = np.concatenate([np.arange(0, 1 << 24, 61, dtype=np.int64), np.arange((1 << 24) - (1 << 18), 1 << 24)])
    q = (x.astype(np.float32) * inv).astype(np.int64)  # x < 2^24: the conversion is exact; truncation
    r = x - q * d
    low, high = r < 0, r >= d
    q, r = q - low + high, r + d * low - d * high
    assert bool(((r >= 0) & (r < d)).all()), "more than one correction step would be needed"
    assert np.array_equal(q, x // d) and np.array_equal(r, x % d)


# ---------------------------------------------------------------------------------------------
# the GEMM file's builders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M,N,impls,splits", gg.SPLIT)
def test_sparse_inputs_keep_every_partial_bf16_exact(T, M, N, impls, splits):
    """<= 32 non-zeros of magnitude <= 2 per dy column against |x| <= 4: |any partial| <= 256; every
    (16-token k-step, 128-column block) is occupied; forced split counts are inside the contracts."""
    dy = gg.sparse_dy(T, M, 1)
    assert gg.sparse_ok(dy) == (True, True)
    assert int((dy != 0).sum(0).min()) == gg.SPARSE_NNZ
    assert gg.SPARSE_NNZ * gg.SPARSE_MAX * gg.V_MAX <= 256
    assert T * gg.SPARSE_MAX * gg.V_MAX + gg.BASE_MAX < gg.LIM
    # a random token subset's partial stays bf16-exact
    x = gg.ints((T, N), gg.V_MAX, 2)
    keep = torch.rand(T, generator=torch.Generator().manual_seed(3)) < 0.5
    part = gg.matmul_ref(dy[keep], x[keep])
    assert float(part.abs().max()) <= 256 and torch.equal(part.float().to(BF16).to(F64), part)
    # removing one occupied k-step changes the result
    gone = dy.clone()
    gone[16 * 5:16 * 6] = 0
    assert gg.first_mismatch(gg.rne_bf16(gg.matmul_ref(gone, x)), gg.rne_bf16(gg.matmul_ref(dy, x))) is not None
    for s in splits:
        assert 1 <= s <= 16
        if 0 in impls:
            assert s <= T // 64 and M % 256 == 0
        if 1 in impls or 2 in impls:
            assert T % 128 == 0 and (T // 128) // s >= 2


def test_dense_table_bounds_and_mismatch_coordinates():
    for T, M, N in gg.DENSE:
        assert T * gg.V_MAX * gg.V_MAX + gg.BASE_MAX < gg.LIM and T % 64 == 0 and M % 128 == 0 and N % 256 == 0
    a = torch.zeros(384, 512, dtype=BF16)
    b = a.clone()
    b[300, 257] = 1.0
    assert gg.first_mismatch(a, a.clone()) is None
    assert gg.first_mismatch(b, a).startswith("first mismatch at tile (1, 1) row 44 column 1 (m 300, n 257)")
    for T, M, N, why in gg.UNSUPPORTED:
        assert T % 64 or N % 256 or M % 128 or (M % 256 == 128 and (T // 64) % 2), why
