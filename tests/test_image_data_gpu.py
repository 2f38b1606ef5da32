"""Image files on the MI355X: the image_batch kernel against its host references — the draw
exactly, the pixels bit for bit, the normalised pixels against float64 — and the device-resident
and host-staged routes of ImageStream against each other.

Cases the draw rule cannot reach at the listed shapes, and where they are tested instead: the area
fraction stays below 1, so at most ONE side of a training crop is clamped to R (asserted: a
full-width or full-height crop) and the full-image crop is the evaluation stream's at R == res
(shape (32, 32)); a side of 1 pixel needs √0.08·R / √(4/3) < 2, i.e. R = 8 (shape (8, 8)).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0xF234_5678_9ABC_DEF1  # high bits set
COPY = ((1.0 / 65536,) * 3, (0.0,) * 3)  # sc, sh under which the output is the four-tap sum / 65536


def _m():
    from paddle_operator_amd import _native
    return _native.require_hip()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _set(n, R, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, R, R, 3), dtype=np.uint8), rng.integers(0, 1000, n).astype(np.int32)


def _launch(img, lab, n, B, R, res, norm, draw, Bg, cuda, staged=False):
    boxes = torch.full((B, 6), -7, dtype=torch.int32, device=cuda)
    x, y = _m().image_batch(torch.from_numpy(img).to(cuda), torch.from_numpy(lab).to(cuda), n, B, R, res, norm, draw,
                            Bg, staged, None, None, boxes)
    assert x.dtype == torch.bfloat16 and tuple(x.shape) == (B, res, res, 3) and y.dtype == torch.int64
    return x.cpu(), y.cpu(), boxes.cpu().numpy().astype(np.int64)


# ----------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("R,res", [(36, 32), (40, 32), (256, 224), (8, 8)])
def test_boxes_match_crop_boxes(cuda, R, res):
    from paddle_operator_amd.data import crop_boxes
    B, rank, n = 257, 3, 1_000_003  # one more row than a block of the boxes kernel
    for stream, m in ((0, 0), (0, 2**32 - 1), (1, 0), (1, 972)):
        out = torch.full((B, 6), -7, dtype=torch.int32, device=cuda)
        assert _m().image_batch(None, None, n, B, R, res, COPY, (SEED, stream, m, rank), 4 * B, False, None, None,
                                out) is None
        want = crop_boxes(SEED, stream, m, rank, B, n, R, res, 4 * B)
        assert np.array_equal(out.cpu().numpy().astype(np.int64), want), (stream, m)
    # stream 1 at m = 972: i = 972·4B + 3B + j = 999 987 + j runs past n = 1 000 003 inside this rank (i = −1)
    assert (want[:, 0] >= 0).any() and (want[:, 0] < 0).any()


# ----------------------------------------------------------------------------- pixels, bit for bit
def _features(bx, R):
    i, x0, y0, cw, ch, flip = bx.T
    return {"side clamped to R": bool(((cw == R) | (ch == R)).any()),
            "right edge": bool(((x0 + cw == R) & (cw < R)).any()),
            "bottom edge": bool(((y0 + ch == R) & (ch < R)).any()),
            "flip": bool(flip.any()), "no flip": bool((flip == 0).any()),
            "upsampled": bool(((cw < 32) | (ch < 32)).any()),
            "one pixel": bool(((cw == 1) | (ch == 1)).any())}


@pytest.mark.parametrize("R,res,B,n", [(36, 32, 3, 5), (40, 32, 5, 2), (256, 224, 2, 3), (8, 8, 64, 3)])
def test_pixels_and_labels_match_the_reference_bit_for_bit(cuda, R, res, B, n):
    from paddle_operator_amd.data import crop_boxes, image_batch_ref
    img, lab = _set(n, R, R * 1000 + B)
    need = {"side clamped to R", "right edge", "bottom edge", "flip", "no flip"} | ({"one pixel"} if R == 8 else set())
    picked, have = [], set()
    for m in range(20000):  # micro-batches whose reference draw adds a wanted case
        new = {k for k, v in _features(crop_boxes(SEED, 0, m, 1, B, n, R, res), R).items() if v} & need - have
        if new or m == 0:
            picked.append(m)
            have |= new
        if have == need:
            break
    assert have == need, need - have
    for m in picked + [2**32 - 1]:
        want_b = crop_boxes(SEED, 0, m, 1, B, n, R, res)
        x, y, boxes = _launch(img, lab, n, B, R, res, COPY, (SEED, 0, m, 1), 2 * B, cuda)
        assert np.array_equal(boxes, want_b), m
        wx, wy = image_batch_ref(img, lab, want_b, res, *COPY)
        assert torch.equal(y, wy) and torch.equal(y, torch.from_numpy(lab[want_b[:, 0]].astype(np.int64))), m
        assert torch.equal(_bits(x), _bits(wx)), (m, want_b.tolist())
        # the staged route: the same draw over the gathered images
        xs, ys, bs = _launch(img[want_b[:, 0]], lab[want_b[:, 0]], n, B, R, res, COPY, (SEED, 0, m, 1), 2 * B, cuda,
                             staged=True)
        assert torch.equal(_bits(xs), _bits(x)) and torch.equal(ys, y) and np.array_equal(bs, boxes), m


def bf16_floor_ceil(v):
    """The largest bf16 ≤ v and the smallest bf16 ≥ v (float64 tensors in, float64 out)."""
    r = v.to(torch.bfloat16)  # a bf16 next to v; its neighbours by ± 1 on the ordered bit patterns
    bits = r.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    key = torch.where(bits < 0x8000, bits, -(bits & 0x7FFF))  # monotonic in the value (−0 → 0)

    def val(k):
        b = torch.where(k >= 0, k, 0x8000 | -k)
        return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.bfloat16).double()
    rd = r.double()
    lo = torch.where(rd > v, val(key - 1), rd)
    hi = torch.where(rd < v, val(key + 1), rd)
    return lo, hi


@pytest.mark.parametrize("R,res,B,n", [(40, 32, 5, 2), (256, 224, 2, 3)])
def test_normalised_pixels_are_bf16_neighbours_of_float64(cuda, R, res, B, n):
    """ImageNet mean / std.  v = sum·sc + sh in float64 (sc, sh the fp32 values the kernel is given).
    The kernel evaluates it with one fp32 multiply and one fp32 add, |error| ≤ e = 2⁻²⁴·(|sum·sc| +
    |v|), then rounds once to bf16: the output must lie between the bf16 below v − e and the bf16
    above v + e.  Away from cancellation (|v| ≫ 2⁹·e) that is exactly "one of the two bf16
    neighbours of v"; the count of outputs outside the plain two neighbours is printed."""
    from paddle_operator_amd.data import _taps, crop_boxes, image_norm
    img, lab = _set(n, R, 7)
    norm = image_norm()
    bx = crop_boxes(SEED, 0, 5, 0, B, n, R, res)
    x, _, boxes = _launch(img, lab, n, B, R, res, norm, (SEED, 0, 5, 0), B, cuda)
    assert np.array_equal(boxes, bx)
    sc, sh = (torch.tensor(a, dtype=torch.float64) for a in norm)
    strict_out = 0
    for j, (i, x0, y0, cw, ch, flip) in enumerate(bx.tolist()):
        iy0, iy1, fy = (torch.from_numpy(a) for a in _taps(ch, res))
        ix0, ix1, fx = (torch.from_numpy(a) for a in _taps(cw, res))
        im = torch.from_numpy(img[i, y0:y0 + ch, x0:x0 + cw].astype(np.int64))
        fy, fx = fy[:, None, None], fx[None, :, None]
        tot = ((256 - fy) * (256 - fx) * im[iy0][:, ix0] + (256 - fy) * fx * im[iy0][:, ix1]
               + fy * (256 - fx) * im[iy1][:, ix0] + fy * fx * im[iy1][:, ix1]).double()
        if flip:
            tot = tot.flip(1)
        v = tot * sc + sh
        e = 2.0 ** -24 * ((tot * sc).abs() + v.abs())
        got = x[j].double()
        lo, hi = bf16_floor_ceil(v - e)[0], bf16_floor_ceil(v + e)[1]
        assert bool(((lo <= got) & (got <= hi)).all()), j
        slo, shi = bf16_floor_ceil(v)
        strict_out += int(((got < slo) | (got > shi)).sum())
    print(f"image-neighbours | R {R} res {res} | outputs outside the two plain neighbours: {strict_out} of {x.numel()}")
    assert strict_out <= x.numel() // 1000  # cancellation is rare


# ----------------------------------------------------------------------------- evaluation stream
@pytest.mark.parametrize("R,res", [(40, 32), (32, 32)])
def test_evaluation_stream_is_a_centre_copy_and_pads(cuda, R, res):
    from paddle_operator_amd.data import crop_boxes
    n, B, world = 11, 4, 2
    img, lab = _set(n, R, 3)
    o = (R - res) // 2
    seen = []
    for m in range(2):
        for rank in range(world):
            x, y, boxes = _launch(img, lab, n, B, R, res, COPY, (SEED, 1, m, rank), world * B, cuda)
            assert np.array_equal(boxes, crop_boxes(SEED, 1, m, rank, B, n, R, res, world * B))
            for j in range(B):
                i = m * world * B + rank * B + j
                if i < n:
                    assert y[j] == lab[i] and np.array_equal(x[j].float().numpy(),
                                                             img[i, o:o + res, o:o + res].astype(np.float32))
                    seen.append(i)
                else:
                    assert y[j] == -1 and not x[j].float().any()
    assert sorted(seen) == list(range(n))


# ----------------------------------------------------------------------------- both routes of ImageStream
def test_staged_and_resident_routes_agree(cuda, tmp_path):
    from paddle_operator_amd.data import EVAL_STREAM, ImageStream
    n, R, res, B = 13, 40, 32, 4
    img, lab = _set(n, R, 11)
    np.save(tmp_path / "images.npy", img)
    np.save(tmp_path / "labels.npy", lab.astype(np.int16))
    kw = dict(seed=SEED, rank=1, world=2)
    dev = ImageStream(str(tmp_path), B, res, 1000, cuda, device_gb=1.0, **kw)
    host = ImageStream(str(tmp_path), B, res, 1000, cuda, device_gb=0.0, **kw)
    assert (dev.placement, host.placement) == ("device", "host")
    try:
        xb = torch.empty(B, res, res, 3, dtype=torch.bfloat16, device=cuda)
        yb = torch.empty(B, dtype=torch.int64, device=cuda)
        for m in (0, 1, 2, 3, 1000, 1001, 2):  # four consecutive micro-batches, a jump ahead, a jump back
            xd, yd = dev.batch(m)
            xh, yh = host.batch(m, out=(xb, yb))
            assert xh.data_ptr() == xb.data_ptr() and yh.data_ptr() == yb.data_ptr()  # the caller's buffers
            wx, wy = dev.host_batch(m)
            assert xd.shape == (B, 3, res, res) and xd.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(_bits(xd.permute(0, 2, 3, 1)), _bits(xh.permute(0, 2, 3, 1))) and torch.equal(yd, yh), m
            assert torch.equal(_bits(xd.permute(0, 2, 3, 1)).cpu(), _bits(wx)) and torch.equal(yd.cpu(), wy), m
        ev = ImageStream(str(tmp_path), B, res, 1000, cuda, device_gb=0.0, stream=EVAL_STREAM, **kw)
        try:
            assert ev.batches_per_epoch() == 2
            x, y = ev.batch(1)  # global rows 12 … 15 of 13 images
            wx, wy = ev.host_batch(1)
            assert y.tolist() == [int(lab[12]), -1, -1, -1] == wy.tolist()
            assert torch.equal(_bits(x.permute(0, 2, 3, 1)).cpu(), _bits(wx))
        finally:
            ev.close()
    finally:
        dev.close()
        host.close()
