// SPDX-License-Identifier: Apache-2.0
// Image batches from a stored uint8 set (gfx950): the random-resized-crop / flip
// sampler of paddle_operator_amd/data.py, the bilinear resample, the per-channel
// normalise, the bf16 NHWC store and the int64 label, one launch.
//
// img is [n][R][R][3] uint8 (RGB, square, R ≤ 4096), lab [n] int32; the output x is
// [B][res][res][3] bf16 (res % 8 == 0, 8 ≤ res ≤ R) and y [B] int64.  Row j of
// micro-batch m is global row g = row0 + j (row0 = rank·B, g < 2³²).  Staged: img is
// a [B][R][R][3] buffer (and lab [B]) gathered on the host and row j reads entry j;
// index, geometry and flip are drawn here all the same, so both routes write the
// same bits.
//
// Draw, stream 0 (training); key = (low, high) words of the data seed, every value an
// unsigned 64-bit integer (the host reference is paddle_operator_amd.data.crop_boxes):
//   A = philox(g, 0, stream, m): i = ((w1 << 32) | w0) mod n, flip = w2 & 1
//   B = philox(g, 1, stream, m) = v0 … v3:
//     f = 5243 + (((v0 >> 16)·60293) >> 16)        area fraction, Q16, in [0.08, 1)
//     s = isqrt((f·R²) << 16)                      side, Q16
//     t = 65536 + (((v1 >> 16)·10138) >> 16)       √ratio, Q16, in [1, √(4/3))
//     a = (s·t) >> 32, b = ((s << 16) / t) >> 16
//     (cw, ch) = v1 & 1 ? (a, b) : (b, a), each clamped to [1, R]
//     x0 = (v2·(R − cw + 1)) >> 32, y0 = (v3·(R − ch + 1)) >> 32
// Stream 1 (evaluation) is not random: i = m·Bglobal + g, the centred res × res box
// (x0 = y0 = (R − res) / 2), no flip; a row with i ≥ n writes label −1 and a zero image.
// boxes_out (optional, int32 [B][6] = i, x0, y0, cw, ch, flip; i = −1 for such a row)
// receives the draw; img == nullptr writes only the boxes.
//
// Resample, signed Q16 source coordinates (x shown; y the same with ch and y0):
//   step = (cw << 16) / res
//   sx = ox·step + (step >> 1) − 32768, clamped to [0, (cw − 1) << 16]
//   ix = sx >> 16, fx = (sx >> 8) & 255, ix1 = min(ix + 1, cw − 1); source column x0 + ix
// and a flipped row writes output column res − 1 − ox.  The four-tap sum
// Σ (256 − fy | fy)(256 − fx | fx)·p is an integer ≤ 255·65536 < 2²⁴, exact in fp32;
// the output is bf16_rne(fl(fl(float(sum)·sc[c]) + sh[c])) — a multiply and an add,
// each rounded (no fma), so the numpy reference has the same bits.  sc = 1/(65536·std),
// sh = −mean/std.  At cw == res the fractions are zero and the kernel is a copy.
//
// One lane owns 8 consecutive output pixels of one row (24 bf16 = three 16-B stores),
// so a wave's reads stay inside a couple of source rows.  The two Philox calls depend
// on the workgroup's image alone (blockIdx.y and kernel arguments): they are uniform
// and run once per wave on the scalar unit, not per lane.  The largest address read is
// img[i][y0 + ch − 1][x0 + cw − 1] with x0 + cw ≤ R and y0 + ch ≤ R.
#include "common.h"
#include "kernels.h"

namespace pdo {

namespace {

struct Box {
  long long i;  // image index; ≥ n only on the evaluation stream
  int x0, y0, cw, ch, flip;
};

// ⌊√x⌋ for x < 2^56, bit by bit (28 steps; per image, not per pixel)
__device__ __forceinline__ unsigned long long isqrt56(unsigned long long x) {
  unsigned long long r = 0;
#pragma unroll 1
  for (int b = 27; b >= 0; --b) {
    const unsigned long long c = r | (1ull << b);
    if (c * c <= x) r = c;
  }
  return r;
}

__device__ __forceinline__ Box draw_box(const DataDraw& d, unsigned long long g, unsigned long long n, int R, int res,
                                        unsigned long long Bglobal) {
  Box bx;
  if (d.stream != 0) {
    bx.i = (long long)((unsigned long long)d.step * Bglobal + g);
    bx.x0 = bx.y0 = (R - res) / 2;
    bx.cw = bx.ch = res;
    bx.flip = 0;
    return bx;
  }
  const Philox4 pa = philox4x32_10((uint32_t)g, 0u, d.stream, d.step, d.key0, d.key1);
  bx.i = (long long)((((unsigned long long)pa.w[1] << 32) | pa.w[0]) % n);
  bx.flip = (int)(pa.w[2] & 1u);
  const Philox4 pb = philox4x32_10((uint32_t)g, 1u, d.stream, d.step, d.key0, d.key1);
  const unsigned long long f = 5243ull + (((unsigned long long)(pb.w[0] >> 16) * 60293ull) >> 16);
  const unsigned long long s = isqrt56((f * (unsigned long long)R * (unsigned long long)R) << 16);
  const unsigned long long t = 65536ull + (((unsigned long long)(pb.w[1] >> 16) * 10138ull) >> 16);
  const unsigned long long a = (s * t) >> 32, b = ((s << 16) / t) >> 16;
  unsigned long long cw = (pb.w[1] & 1u) ? a : b, ch = (pb.w[1] & 1u) ? b : a;
  cw = cw < 1 ? 1 : (cw > (unsigned long long)R ? (unsigned long long)R : cw);
  ch = ch < 1 ? 1 : (ch > (unsigned long long)R ? (unsigned long long)R : ch);
  bx.cw = (int)cw;
  bx.ch = (int)ch;
  bx.x0 = (int)(((unsigned long long)pb.w[2] * (unsigned long long)(R - bx.cw + 1)) >> 32);
  bx.y0 = (int)(((unsigned long long)pb.w[3] * (unsigned long long)(R - bx.ch + 1)) >> 32);
  return bx;
}

__device__ __forceinline__ void write_box(int* __restrict__ out, const Box& bx, unsigned long long n) {
  out[0] = (unsigned long long)bx.i < n ? (int)bx.i : -1;
  out[1] = bx.x0;
  out[2] = bx.y0;
  out[3] = bx.cw;
  out[4] = bx.ch;
  out[5] = bx.flip;
}

__global__ __launch_bounds__(256) void image_boxes_kernel(long long n, int B, int R, int res, DataDraw d,
                                                          unsigned long long Bglobal, int* __restrict__ boxes_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= B) return;
  write_box(boxes_out + (size_t)j * 6, draw_box(d, d.row0 + (unsigned long long)j, (unsigned long long)n, R, res, Bglobal),
            (unsigned long long)n);
}

// fl(fl(a·b) + c): two roundings, never contracted into an fma (the header's rule)
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p + c;
}

// source index and the weight of its right / lower neighbour along one axis
__device__ __forceinline__ void tap(int o, int step, int c, int& i0, int& i1, int& f) {
  int s = o * step + (step >> 1) - 32768;
  const int hi = (c - 1) << 16;
  s = s < 0 ? 0 : (s > hi ? hi : s);
  i0 = s >> 16;
  f = (s >> 8) & 255;
  i1 = i0 + 1 < c ? i0 + 1 : c - 1;
}

// grid (⌈res·res/8 / 256⌉, B): lane task t = (output row oy, group of 8 output columns)
template <bool STAGED>
__global__ __launch_bounds__(256) void image_batch_kernel(const uint8_t* __restrict__ img, const int* __restrict__ lab,
                                                          long long n, int R, int res, ImageNorm nm,
                                                          bf16* __restrict__ x, int64_t* __restrict__ y, DataDraw d,
                                                          unsigned long long Bglobal, int* __restrict__ boxes_out) {
  const int j = blockIdx.y;
  const Box bx = draw_box(d, d.row0 + (unsigned long long)j, (unsigned long long)n, R, res, Bglobal);
  const bool live = (unsigned long long)bx.i < (unsigned long long)n;
  const long long src = STAGED ? (long long)j : bx.i;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    y[j] = live ? (int64_t)lab[src] : (int64_t)-1;
    if (boxes_out != nullptr) write_box(boxes_out + (size_t)j * 6, bx, (unsigned long long)n);
  }
  const int G8 = res / 8;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= res * G8) return;
  const int oy = t / G8, oc0 = (t - oy * G8) * 8;
  bf16x8* out = reinterpret_cast<bf16x8*>(x + (((long long)j * res + oy) * res + oc0) * 3);
  if (!live) {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    out[0] = z;
    out[1] = z;
    out[2] = z;
    return;
  }
  const int stepx = (bx.cw << 16) / res, stepy = (bx.ch << 16) / res;
  int iy0, iy1, fy;
  tap(oy, stepy, bx.ch, iy0, iy1, fy);
  const uint8_t* base = img + (size_t)src * R * R * 3;
  const uint8_t* r0 = base + ((size_t)(bx.y0 + iy0) * R + bx.x0) * 3;
  const uint8_t* r1 = base + ((size_t)(bx.y0 + iy1) * R + bx.x0) * 3;
  float v[24];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int oc = oc0 + k;
    int ix0, ix1, fx;
    tap(bx.flip ? res - 1 - oc : oc, stepx, bx.cw, ix0, ix1, fx);
    const int w00 = (256 - fy) * (256 - fx), w01 = (256 - fy) * fx, w10 = fy * (256 - fx), w11 = fy * fx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int sum = w00 * r0[ix0 * 3 + c] + w01 * r0[ix1 * 3 + c] + w10 * r1[ix0 * 3 + c] + w11 * r1[ix1 * 3 + c];
      v[k * 3 + c] = mul_then_add((float)sum, nm.sc[c], nm.sh[c]);
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    f32x8 f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = v[q * 8 + e];
    out[q] = to_bf16(f);
  }
}

}  // namespace

int image_batch(const uint8_t* img, const int* lab, long long n, int B, int R, int res, const ImageNorm& nm, bf16* x,
                int64_t* y, const DataDraw& draw, long long Bglobal, bool staged, int* boxes_out, hipStream_t st) {
  if (B < 1 || B > 65535 || R < 8 || R > 4096 || res < 8 || res > R || res % 8 != 0 || n < 1) return -2;
  if (n > (1ll << 31) - 1 || Bglobal < 1 || Bglobal > (1ll << 31)) return -3;
  if (draw.stream > 1 || draw.row0 + (unsigned long long)B > (1ull << 32)) return -4;  // g < 2^32
  if (img == nullptr) {  // boxes only
    if (boxes_out == nullptr) return -5;
    image_boxes_kernel<<<(B + 255) / 256, 256, 0, st>>>(n, B, R, res, draw, (unsigned long long)Bglobal, boxes_out);
    return 0;
  }
  if (lab == nullptr || x == nullptr || y == nullptr) return -5;
  const dim3 grid((unsigned)((res * (res / 8) + 255) / 256), (unsigned)B);
  if (staged)
    image_batch_kernel<true><<<grid, 256, 0, st>>>(img, lab, n, R, res, nm, x, y, draw, (unsigned long long)Bglobal,
                                                   boxes_out);
  else
    image_batch_kernel<false><<<grid, 256, 0, st>>>(img, lab, n, R, res, nm, x, y, draw, (unsigned long long)Bglobal,
                                                    boxes_out);
  return 0;
}

}  // namespace pdo
