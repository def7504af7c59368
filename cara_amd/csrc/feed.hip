// The training feed's patch rows (gfx950 only): images -> rows bf16 [B*gh*gw, C*p*p] of the patch-embedding GEMM, column =
// (c*p + py)*p + px (the flattening of Conv2d weight [D, C, p, p]), from an fp32 batch or straight from resident uint8 pixels --
// whole images or a crop box per sample, RandAugment's affine and lookup ops, Mixup / CutMix, colour jitter and Random Erasing by
// index, all rows or a kept subset.
// One call is one cara_feed (common.h); cara_feed_patch_rows checks it and launches one of TWO kernel bodies:
//   aligned_rows_kernel<T, KEEP>        the source is the output's size and dword-aligned: one float4 / one dword per lane
//   box_rows<MIX, AUG, RA, KEEP>        the source is read through a box: byte loads for four adjacent pixels, one 8-byte store
// What a body CAN meet is a template parameter, so an instantiation carries nothing of a feature it does not have (the crop form no
// partner, the mix form no jitter row, none but the RA forms a RandAugment row); what a lane is (feed_lane: its row, its sample, its
// refusal) is one text for all of them.  box_rows is entered through box_rows_kernel<MIX, AUG, KEEP> (RA = false: the kernels'
// names are what they were, so a host trace of a call without the ra table is the one it was) and box_rows_ra_kernel<AUG, KEEP>.
// The next feed feature is a field of cara_feed and a parameter of a body, not a sibling kernel.
#include <type_traits>

#include "common.h"

namespace {

// ToTensor + Normalize of vtab.py:92-94 on resident uint8 pixels, in the fp32 operation order of data.normalize_u8 -- u / 255,
// - mean[c], / std[c], two correctly rounded divisions (no reciprocal multiply: the build has no fast-math flag) -- then the one
// rounding to the build's 16-bit type that the fp32 source gets.  The fp32 image tensor is never written.  Four pixels (one dword).
__device__ __forceinline__ bf16x4 normalize_u8x4(unsigned u, float mu, float sd) {
  const float v0 = ((float)(u & 255u) / 255.0f - mu) / sd;
  const float v1 = ((float)((u >> 8) & 255u) / 255.0f - mu) / sd;
  const float v2 = ((float)((u >> 16) & 255u) / 255.0f - mu) / sd;
  const float v3 = ((float)(u >> 24) / 255.0f - mu) / sd;
  return bf16x4{(bf16)v0, (bf16)v1, (bf16)v2, (bf16)v3};
}

// A crop box per sample: pixels [n_split,C,Hs,Ws] of any size, boxes int32 [B,5] = (x0, y0, w, h, flip) in source pixels.  Output
// pixel (oy, ox) is the bilinear sample (half-pixel centres, no antialiasing filter: what F.interpolate(crop, (Hi,Wi), "bilinear",
// align_corners=False) gives) of the box at ox' = flip ? Wi-1-ox : ox, with indices clamped inside the box.  Each axis is evaluated
// as a + f * (b - a): the same polynomial as (1-f) a + f b, and exact where f == 0 or a == b -- a box of the output's size gives the
// source bytes themselves and a 1x1 box a constant image, bit for bit what normalize_u8x4 gives for that byte.  The source is
// fetched with byte loads: the box starts at any byte and Ws need not be a multiple of 4, so no dword of the source is aligned;
// neighbouring lanes read neighbouring bytes of the same two source rows.
struct CropAxis { int i0, i1; float f; };
__device__ __forceinline__ CropAxis crop_axis(int o, int n_out, int n_box, bool flip) {
  const int of = flip ? n_out - 1 - o : o;
  const float s = fmaxf(((float)of + 0.5f) * ((float)n_box / (float)n_out) - 0.5f, 0.0f);
  const int i0 = min((int)s, n_box - 1);
  return CropAxis{i0, min(i0 + 1, n_box - 1), s - (float)i0};
}
// normalize_u8x4's operations on a value that is no longer a byte
__device__ __forceinline__ float normalize_f32(float v, float mu, float sd) { return (v / 255.0f - mu) / sd; }
// the bilinear value of one output pixel, before normalisation: top / bot = the two source rows at the box's left edge
__device__ __forceinline__ float crop_value(const uint8_t* top, const uint8_t* bot, const CropAxis& ax, float fy) {
  const float t0 = (float)top[ax.i0], t1 = (float)top[ax.i1], b0 = (float)bot[ax.i0], b1 = (float)bot[ax.i1];
  const float t = t0 + ax.f * (t1 - t0), u = b0 + ax.f * (b1 - b0);
  return t + fy * (u - t);
}
// What sample b reads: image rows[b] of the split, whole (boxes NULL: the host then asks Hs == Hi, Ws == Wi) or through its box.
// false, and nothing formed from it, for a row outside [0, n_split) or a box not inside the source.
struct MixSource { const uint8_t* origin; int w, h; bool flip; };   // byte (y0, x0) of channel 0 of the image, and its box
__device__ __forceinline__ bool mix_source(const uint8_t* img, long n_split, int C, int Hs, int Ws, const int64_t* rows,
                                           const int* boxes, int b, MixSource* s) {
  const int64_t r = rows[b];
  int x0 = 0, y0 = 0, w = Ws, h = Hs, flip = 0;
  if (boxes) {
    const int* box = boxes + (size_t)b * 5;
    x0 = box[0]; y0 = box[1]; w = box[2]; h = box[3]; flip = box[4];
  }
  // (x0, y0 >= 0 is checked before Ws - x0, Hs - y0 are formed: no overflow for any int)
  if (r < 0 || r >= n_split || w < 1 || h < 1 || x0 < 0 || y0 < 0 || w > Ws - x0 || h > Hs - y0) return false;
  *s = MixSource{img + (size_t)r * C * Hs * Ws + (size_t)y0 * Ws + x0, w, h, flip != 0};
  return true;
}
// the two source rows of channel 0 that one output row of a sample reads, and what crop_axis needs for its columns
struct RowSource { const uint8_t *top, *bot; size_t plane; float fy; int w; bool flip; };
__device__ __forceinline__ RowSource row_source(const MixSource& s, int oy, int Hi, int Hs, int Ws) {
  const CropAxis ay = crop_axis(oy, Hi, s.h, false);
  return RowSource{s.origin + (size_t)ay.i0 * Ws, s.origin + (size_t)ay.i1 * Ws, (size_t)Hs * Ws, ay.f, s.w, s.flip};
}

// Mixup / CutMix: mix int32 [B,8] = (partner, cx0, cy0, cw, ch, blend, target, 0).  Sample b is mixed with what sample `partner`
// would be UNMIXED at the same output position (through rows[partner] and boxes[partner], its flip included, after ITS OWN jitter
// chain where there is one): inside the rectangle (cx0, cy0, cw, ch) of the output the pixel is the partner's, outside it
// a + m (b - a) on the un-normalised 0..255 values, m = the fp32 whose bits `blend` holds -- exact at m == 0, like the axes'
// a + f (b - a).  Then normalize_f32 and the one rounding to 16 bits.  `target` is the loss's (xent_mix_kernel).  A pixel loads only
// the image it needs -- the partner alone inside the rectangle, its own alone outside it when m == 0 -- and a sample that is its
// own partner checks one source, not two: an identity table costs the plain call's loads plus its table row.  No table (NULL, or a
// body that takes none): every sample is its own partner with an empty rectangle and m == 0.  OPTIONAL: the table may be NULL (the
// jitter form's; the mix form is chosen because the table is there and does not ask).
struct MixRow { int partner, cx0, cy0, cw, ch; float m; };
template <bool MIX, bool OPTIONAL>
__device__ __forceinline__ MixRow mix_row(const int* mix, int b) {
  MixRow r{b, 0, 0, 0, 0, 0.0f};
  if (MIX && (!OPTIONAL || mix)) {
    const int* mx = mix + (size_t)b * 8;
    r = MixRow{mx[0], mx[1], mx[2], mx[3], mx[4], __int_as_float(mx[5])};
  }
  return r;
}
// (cx0, cy0 >= 0 before Wi - cx0, Hi - cy0 are formed; a NaN fails m >= 0)
__device__ __forceinline__ bool mix_row_ok(const MixRow& r, int Hi, int Wi) {
  return r.cw >= 0 && r.ch >= 0 && r.cx0 >= 0 && r.cy0 >= 0 && r.cw <= Wi - r.cx0 && r.ch <= Hi - r.cy0 && r.m >= 0.0f && r.m <= 1.0f;
}
// the Mixup blend (crop_value's argument)
__device__ __forceinline__ float mix_blend(float a, float m, float b) { return a + m * (b - a); }

// Colour jitter and Random Erasing by index: aug int32 [B,16], row b =
//   (op0, f0, op1, f1, op2, f2, ex0, ey0, ew, eh, emode, eseed, 0, 0, 0, 0)
// op: 0 none, 1 brightness, 2 contrast, 3 saturation, each non-zero code at most once in a row, any order (torchvision's
// ColorJitter draws a permutation); f: the bits of a finite fp32 factor >= 0 (not read where op == 0); (ex0, ey0, ew, eh): the erase
// rectangle in output pixels (ew == 0 or eh == 0: none); emode 0 const, 1 pixel; eseed any 32 bits; the last four words 0.
// All arithmetic below is fp32, every product and sum a single IEEE operation (plain operators under `fp contract(off)`), on the
// un-normalised 0..255 values.  With u = a sample's own unmixed bilinear value (crop_value):
//   slot k = 0, 1, 2 in order:   v <- min(max(f v + (1 - f) d, 0), 255)       two products, one sum, and 1 - f rounded once
//     brightness: d = 0;   saturation: d = gray = (0.2989 r + 0.587 g) + 0.114 b of THAT pixel's three channel values as they
//     stand at that slot (three products, two sums, left to right);   contrast: d = M_b, the mean of gray over all Hi x Wi output
//     pixels of sample b's image as it stands before the contrast slot (aug_gray_mean_kernel).
//   torchvision's _blend on float tensors, rescaled to 0..255: exact at f == 1 (1 v + 0 d = v), d clamped at f == 0.
//   Then the mix step, exactly: inside the CutMix rectangle the partner's value, outside it a + m (b - a) -- the partner's
//   value being the partner's unmixed value after ITS OWN chain (its table row, its M).  Then normalize_f32.
//   Then the erase: inside (ex0, ey0, ew, eh) the normalised value is replaced by 0 (const) or by a standard normal z (pixel: timm's
//   RandomErasing(mode="pixel"), one rectangle):  i = ((b C + c) Hi + oy) Wi + ox, the element's index in [B,C,Hi,Wi];
//     h1 = keep_hash(2 i, eseed, AUG_ERASE_STREAM),  h2 = keep_hash(2 i + 1, eseed, AUG_ERASE_STREAM);
//     u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1],  u2 = (h2 >> 8) 2^-24 in [0, 1)                    (both exact)
//     z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2): roundings at logf, the product with -2 (exact), sqrtf, the product 2 pi u2, cosf
//     and the last product.  The host refuses 2 B C Hi Wi > 2^32.
//   Then the one rounding to the build's 16-bit type.
// Strict rule: nothing overflows and nothing is formed from an unchecked value.  An op outside [0, 3], a repeated op, a factor that
// is negative, infinite or NaN, a rectangle not inside the output (ew, eh >= 0, ex0, ey0 >= 0, ew <= Wi - ex0, eh <= Hi - ey0: the
// CutMix order), emode outside {0, 1} or a non-zero pad word make the row bad.  C == 3 (the host refuses any other count).  A lane
// loads the other two channels only where a saturation slot is present, and a sample whose row is all zero does the mix form's
// loads plus its 64-byte table row.
constexpr int AUG_GROUPS = 16;                        // workgroups per sample in aug_gray_mean_kernel (fixed: part of the tree)
constexpr unsigned AUG_ERASE_STREAM = 0x45524153u;    // keep_hash stream of the erase noise
struct AugRow { int op[3]; float f[3]; int ex0, ey0, ew, eh, emode; unsigned eseed; int contrast_at; bool sat; };
__device__ __forceinline__ bool aug_row(const int* aug, int b, int Hi, int Wi, AugRow* a) {
  const int* r = aug + (size_t)b * 16;
  bool ok = true;
  int seen = 0;
  a->contrast_at = 3;
  a->sat = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int op = r[2 * k];
    float f = 0.0f;
    if (op < 0 || op > 3) ok = false;
    else if (op != 0) {
      f = __int_as_float(r[2 * k + 1]);
      if ((seen >> op) & 1) ok = false;
      seen |= 1 << op;
      if (!(f >= 0.0f && f <= 3.402823466e38f)) ok = false;   // (a NaN fails f >= 0)
      if (op == 2) a->contrast_at = k;
      if (op == 3) a->sat = true;
    }
    a->op[k] = op;
    a->f[k] = f;
  }
  a->ex0 = r[6]; a->ey0 = r[7]; a->ew = r[8]; a->eh = r[9]; a->emode = r[10]; a->eseed = (unsigned)r[11];
  // (ex0, ey0 >= 0 before Wi - ex0, Hi - ey0 are formed)
  return ok && a->ew >= 0 && a->eh >= 0 && a->ex0 >= 0 && a->ey0 >= 0 && a->ew <= Wi - a->ex0 && a->eh <= Hi - a->ey0 &&
         (a->emode == 0 || a->emode == 1) && (r[12] | r[13] | r[14] | r[15]) == 0;
}
__device__ __forceinline__ float aug_gray(float r, float g, float b) {
#pragma clang fp contract(off)
  return (0.2989f * r + 0.587f * g) + 0.114f * b;
}
__device__ __forceinline__ float aug_blend(float v, float d, float f, float omf) {
#pragma clang fp contract(off)
  return fminf(fmaxf(f * v + omf * d, 0.0f), 255.0f);
}
// slots [0, upto) of a row on one pixel: THREE: on its three channel values; otherwise on r alone (no saturation slot among them)
template <bool THREE>
__device__ __forceinline__ void aug_chain(float& r, float& g, float& b, const AugRow& a, int upto, float M) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int op = a.op[k];
    if (k >= upto || op == 0) continue;
    const float f = a.f[k], omf = 1.0f - f;
    const float d = op == 3 ? aug_gray(r, g, b) : (op == 2 ? M : 0.0f);
    r = aug_blend(r, d, f, omf);
    if (THREE) {
      g = aug_blend(g, d, f, omf);
      b = aug_blend(b, d, f, omf);
    }
  }
}
__device__ __forceinline__ float aug_noise(unsigned i, unsigned seed) {
#pragma clang fp contract(off)
  const unsigned h1 = keep_hash(2u * i, seed, AUG_ERASE_STREAM), h2 = keep_hash(2u * i + 1u, seed, AUG_ERASE_STREAM);
  const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-8f, u2 = (float)(h2 >> 8) * 5.9604644775390625e-8f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}
// channel c of one output pixel after the sample's own chain; base(ch) = channel ch of that pixel before the chain
template <class Base>
__device__ __forceinline__ float aug_value(Base&& base, const AugRow& a, float M, int c) {
  if (a.sat) {
    float r = base(0), g = base(1), b = base(2);
    aug_chain<true>(r, g, b, a, 3, M);
    return c == 0 ? r : (c == 1 ? g : b);
  }
  float v = base(c), g = 0.0f, b = 0.0f;
  aug_chain<false>(v, g, b, a, 3, M);
  return v;
}

// RandAugment by index: ra int32 [B,16], row b =
//   (op0, arg0, op1, arg1, op2, arg2, m00, m01, m02, m10, m11, m12, fill, 0, 0, 0)
// op: a lookup slot on the quantised value q, applied in the order 0, 1, 2:
//   0 none (arg 0);   1 posterize, arg = bits kept 0..8: q & ~((1 << (8 - arg)) - 1);   2 solarize, arg = threshold 0..256:
//   q < arg ? q : 255 - q;   3 solarize-add, arg 0..255: q < 128 ? min(q + arg, 255) : q;   4 invert: 255 - q (arg 0);
//   5 autocontrast, 6 equalize (arg 0): the sample's channel table, at most one of the two in a row (ra_table_kernel).
// m..: the bits of six finite fp32 numbers of magnitude <= 32768, the output-to-input affine;  fill = 0x00RRGGBB.
// All arithmetic below is fp32, every product and sum a single IEEE operation (plain operators under `fp contract(off)`).  Output
// pixel (ox, oy), x = ox + 0.5, y = oy + 0.5:   u = (m00 x + m01 y) + m02,   v = (m10 x + m11 y) + m12.
//   Unless 0 <= u < Wi and 0 <= v < Hi (a NaN fails; nothing is converted to an integer before the test) the value is the fill byte
//   of the channel.  Inside, the sample's box (w x h, flip) is sampled at the continuous position:
//     uf = flip ? Wi - u : u,  s = max(uf (w / Wi) - 0.5, 0),  i0 = min((int)s, w - 1),  i1 = min(i0 + 1, w - 1),  f = s - i0;
//     the same for v with h / Hi and no flip;  then t + fy (b - t) of the two rows' a + f (b - a).
//   A row whose matrix words are the bits of (1, 0, 0, 0, 1, 0) takes crop_axis / crop_value instead: bit for bit the value of the
//   call without the table, with that code's contraction.
//   Where the row has a lookup slot: q = (int)rintf(value) (half to even; the value is in [0, 255]), the slots on q, and (float)q
//   goes on -- the fill pixels too.  A row without one does not quantise.
//   Then the jitter chain of the aug row where there is one, the mix, normalize_f32, the erase, the one rounding to 16 bits: the
//   value above stands where crop_value stood.
// The statistic slot: h_c[256] = the histogram of q, as it stands before that slot, over ALL Hi x Wi output pixels of the sample's
// channel c (fill pixels count; patch dropout does not change it).  Integers: no order of summation matters.
//   ra_hist_kernel: RA_GROUPS workgroups of 256 threads per sample, LDS atomics into int [3][256], stored whole as the workgroup's
//     partial (nothing of the scratch is read before it is written: its earlier content does not matter);
//   ra_table_kernel: one workgroup per (sample, channel), thread i = bin i: h[i] = the sum of the partials, then
//     autocontrast: lo, hi = first and last non-zero bin; hi <= lo: identity; else lut[i] = clamp((255 (i - lo)) / (hi - lo), 0, 255)
//       in integer division, 0 below lo;
//     equalize: z = h[hi], step = (sum h - z) / 255; hi <= lo or step == 0: identity; else lut[i] = min(255, (step / 2 +
//       sum_{j < i} h[j]) / step).
// scratch: lut uint8 [B][3][256], then partial int32 [B][RA_GROUPS][3][256] (cara_ra_stat_bytes).  A sample without a statistic slot
// or with a bad row loads no pixel and writes nothing; one whose source is bad writes zero partials (an identity table nobody reads).
// Strict rule: an op outside [0, 6], an argument outside its range, two statistic slots, a matrix word that is not finite or larger
// than 32768 in magnitude, a fill with a non-zero top byte or a non-zero pad word make the row bad.  C == 3.
constexpr int RA_GROUPS = 8;                          // workgroups per sample in ra_hist_kernel
struct RaRow { int slot[3]; float m[6]; int fill, stat_at, stat_op; bool ident, lookup; };   // slot = op | arg << 4
__device__ __forceinline__ bool ra_row(const int* ra, int b, RaRow* r) {
  const int* w = ra + (size_t)b * 16;
  bool ok = true;
  r->stat_at = 3;
  r->stat_op = 0;
  r->lookup = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int op = w[2 * k], arg = w[2 * k + 1];
    const int top = op == 1 ? 8 : (op == 2 ? 256 : (op == 3 ? 255 : 0));
    if (op < 0 || op > 6 || arg < 0 || arg > top) ok = false;
    if (op == 5 || op == 6) {
      if (r->stat_at != 3) ok = false;
      r->stat_at = k;
      r->stat_op = op;
    }
    if (op != 0) r->lookup = true;
    r->slot[k] = op | (arg << 4);   // (used only where ok)
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    r->m[i] = __int_as_float(w[6 + i]);
    if (!(fabsf(r->m[i]) <= 32768.0f)) ok = false;   // (a NaN fails)
  }
  r->ident = w[6] == 0x3f800000 && w[7] == 0 && w[8] == 0 && w[9] == 0 && w[10] == 0x3f800000 && w[11] == 0;
  r->fill = w[12];
  return ok && ((unsigned)r->fill >> 24) == 0 && (w[13] | w[14] | w[15]) == 0;
}
// lookup slots [0, upto) on a quantised value; lut: the sample's table of that channel (read at the statistic slot alone)
__device__ __forceinline__ int ra_slots(int q, const RaRow& r, const uint8_t* lut, int upto) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int op = r.slot[k] & 15, arg = r.slot[k] >> 4;
    if (k >= upto || op == 0) continue;
    if (op == 1) q &= ~((1 << (8 - arg)) - 1);
    else if (op == 2) q = q < arg ? q : 255 - q;
    else if (op == 3) q = q < 128 ? min(q + arg, 255) : q;
    else if (op == 4) q = 255 - q;
    else q = lut[q];
  }
  return q;
}
// the continuous position's bilinear value (or the fill byte) of channel c of output pixel (ox, oy); plane = Hs Ws
__device__ __forceinline__ float ra_geometry(const MixSource& s, const RaRow& r, int c, int ox, int oy, int Hi, int Wi, int Ws, size_t plane) {
#pragma clang fp contract(off)
  const float x = (float)ox + 0.5f, y = (float)oy + 0.5f;
  const float u = (r.m[0] * x + r.m[1] * y) + r.m[2];
  const float v = (r.m[3] * x + r.m[4] * y) + r.m[5];
  if (!(u >= 0.0f && u < (float)Wi && v >= 0.0f && v < (float)Hi)) return (float)((r.fill >> (16 - 8 * c)) & 255);
  const float uf = s.flip ? (float)Wi - u : u;
  const float sx = fmaxf(uf * ((float)s.w / (float)Wi) - 0.5f, 0.0f), sy = fmaxf(v * ((float)s.h / (float)Hi) - 0.5f, 0.0f);
  const int x0 = min((int)sx, s.w - 1), x1 = min(x0 + 1, s.w - 1), y0 = min((int)sy, s.h - 1), y1 = min(y0 + 1, s.h - 1);
  const float fx = sx - (float)x0, fy = sy - (float)y0;
  const uint8_t *top = s.origin + c * plane + (size_t)y0 * Ws, *bot = s.origin + c * plane + (size_t)y1 * Ws;
  const float t0 = (float)top[x0], t1 = (float)top[x1], b0 = (float)bot[x0], b1 = (float)bot[x1];
  const float t = t0 + fx * (t1 - t0), bb = b0 + fx * (b1 - b0);
  return t + fy * (bb - t);
}
// channel c of output pixel (ox, oy) of a sample after its ra row: the geometry, then the lookup slots [0, upto).  ident(c): that
// channel by crop_value (the call without the table); lut: the sample's tables [3][256]
template <class Ident>
__device__ __forceinline__ float ra_value(const MixSource& s, const RaRow& r, const uint8_t* lut, int c, int ox, int oy, int Hi, int Wi,
                                          int Ws, size_t plane, int upto, Ident&& ident) {
  float v = r.ident ? ident(c) : ra_geometry(s, r, c, ox, oy, Hi, Wi, Ws, plane);
  if (r.lookup) v = (float)ra_slots(min(max((int)rintf(v), 0), 255), r, lut + c * 256, upto);
  return v;
}
// ra_value where no lane keeps a row pair: the pre-passes, one pixel at a time
__device__ __forceinline__ float ra_pixel(const MixSource& s, const RaRow& r, const uint8_t* lut, int c, int ox, int oy, int Hi, int Wi,
                                          int Hs, int Ws, int upto) {
  return ra_value(s, r, lut, c, ox, oy, Hi, Wi, Ws, (size_t)Hs * Ws, upto, [&](int ch) {
    const RowSource src = row_source(s, oy, Hi, Hs, Ws);
    return crop_value(src.top + ch * src.plane, src.bot + ch * src.plane, crop_axis(ox, Wi, src.w, src.flip), src.fy);
  });
}

__global__ __launch_bounds__(256) void ra_hist_kernel(const uint8_t* __restrict__ img, long n_split, int Hs, int Ws,
                                                      const int64_t* __restrict__ rows, const int* __restrict__ boxes,
                                                      const int* __restrict__ ra, int* __restrict__ partial, int B, int C, int Hi, int Wi) {
  __shared__ int h[3 * 256];
  const int b = blockIdx.x / RA_GROUPS, k = blockIdx.x % RA_GROUPS;
  RaRow r;
  if (!ra_row(ra, b, &r) || r.stat_at == 3) return;
  int* out = partial + ((size_t)b * RA_GROUPS + k) * (3 * 256);
  MixSource s;
  const bool src_ok = mix_source(img, n_split, C, Hs, Ws, rows, boxes, b, &s);
  for (int i = threadIdx.x; i < 3 * 256; i += 256) h[i] = 0;
  __syncthreads();
  if (src_ok) {
    const int n = Hi * Wi;
    for (int q = k * 256 + (int)threadIdx.x; q < n; q += 256 * RA_GROUPS) {
      const int oy = q / Wi, ox = q - oy * Wi;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // (the row has a lookup slot: ra_value quantised, and slots keep [0, 255])
        const int v = (int)ra_pixel(s, r, nullptr, c, ox, oy, Hi, Wi, Hs, Ws, r.stat_at);
        atomicAdd(&h[c * 256 + min(max(v, 0), 255)], 1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 256; i += 256) out[i] = h[i];
}
__global__ __launch_bounds__(256) void ra_table_kernel(const int* __restrict__ ra, const int* __restrict__ partial,
                                                       uint8_t* __restrict__ lut, int B) {
  __shared__ int h[256];
  __shared__ int lo, hi;
  const int b = blockIdx.x / 3, c = blockIdx.x % 3, i = threadIdx.x;
  RaRow r;
  if (!ra_row(ra, b, &r) || r.stat_at == 3) return;
  int mine = 0;
  for (int k = 0; k < RA_GROUPS; ++k) mine += partial[((size_t)b * RA_GROUPS + k) * (3 * 256) + c * 256 + i];
  h[i] = mine;
  if (i == 0) { lo = 256; hi = -1; }
  __syncthreads();
  if (mine != 0) { atomicMin(&lo, i); atomicMax(&hi, i); }
  __syncthreads();
  int v = i;
  if (hi > lo) {
    if (r.stat_op == 5) {
      v = i < lo ? 0 : min(255 * (i - lo) / (hi - lo), 255);
    } else {
      int before = 0, total = 0;
      for (int j = 0; j < 256; ++j) {
        if (j == i) before = total;
        total += h[j];
      }
      const int step = (total - h[hi]) / 255;
      if (step != 0) v = min(255, (step / 2 + before) / step);
    }
  }
  lut[((size_t)b * 3 + c) * 256 + i] = (uint8_t)v;
}

// The pre-pass of the contrast slot: M_b = the mean of gray over the Hi x Wi output pixels of sample b after the slots that precede
// its contrast slot, through a FIXED tree (docs/findings/optimizer_side.md section 2's manner; no atomics).  AUG_GROUPS workgroups
// of 256 threads per sample, whatever the image size:
//   1. thread t of workgroup k: acc = 0; for q = 256 k + t, + 256 AUG_GROUPS, ... < Hi Wi: acc = acc + gray(pixel q), q = oy Wi + ox;
//   2. the wave's 64 accumulators by wave_sum's butterfly (lanes 32, 16, 8, 4, 2, 1 apart): 6 additions;
//   3. the four wave sums left to right: 3 additions                                       -> partial[b][k]
//   4. aug_gray_mean_reduce_kernel, one thread per sample: the AUG_GROUPS partials left to right (15 additions), then one division
//      by (float)(Hi Wi)                                                                    -> stat[b]
// A sample whose row is bad or has no contrast slot loads no pixel and writes nothing; one whose source is bad writes zero partials
// (the patch-row kernel never reads its stat).  scratch: stat fp32 [B], then partial fp32 [B][AUG_GROUPS] (cara_aug_stat_bytes).
// M_b is the mean over the whole image, whether its patches are all kept or not.
// RA (aug_gray_mean_ra_kernel): the three channel values are the sample's values after its ra row (ra_pixel, behind ra_table_kernel);
// a bad ra row writes zero partials like a bad source.
template <bool RA>
__device__ __forceinline__ void aug_gray_mean(const uint8_t* __restrict__ img, long n_split, int Hs, int Ws, const int64_t* __restrict__ rows,
                                              const int* __restrict__ boxes, const int* __restrict__ aug, const int* __restrict__ ra,
                                              const uint8_t* __restrict__ lut, float* __restrict__ partial, int B, int C, int Hi, int Wi) {
#pragma clang fp contract(off)
  __shared__ float lds[4];
  const int b = blockIdx.x / AUG_GROUPS, k = blockIdx.x % AUG_GROUPS;
  AugRow a;
  if (!aug_row(aug, b, Hi, Wi, &a) || a.contrast_at == 3) return;
  MixSource s;
  RaRow rr;
  bool ok = mix_source(img, n_split, C, Hs, Ws, rows, boxes, b, &s);
  if constexpr (RA) ok = ra_row(ra, b, &rr) && ok;
  if (!ok) {
    if (threadIdx.x == 0) partial[(size_t)b * AUG_GROUPS + k] = 0.0f;
    return;
  }
  float acc = 0.0f;
  const int n = Hi * Wi;
  for (int q = k * 256 + (int)threadIdx.x; q < n; q += 256 * AUG_GROUPS) {
    const int oy = q / Wi, ox = q - oy * Wi;
    float r, g, bl;
    if constexpr (RA) {
      const uint8_t* t = lut + (size_t)b * (3 * 256);
      r = ra_pixel(s, rr, t, 0, ox, oy, Hi, Wi, Hs, Ws, 3);
      g = ra_pixel(s, rr, t, 1, ox, oy, Hi, Wi, Hs, Ws, 3);
      bl = ra_pixel(s, rr, t, 2, ox, oy, Hi, Wi, Hs, Ws, 3);
    } else {
      const RowSource src = row_source(s, oy, Hi, Hs, Ws);
      const CropAxis ax = crop_axis(ox, Wi, src.w, src.flip);
      r = crop_value(src.top, src.bot, ax, src.fy);
      g = crop_value(src.top + src.plane, src.bot + src.plane, ax, src.fy);
      bl = crop_value(src.top + 2 * src.plane, src.bot + 2 * src.plane, ax, src.fy);
    }
    aug_chain<true>(r, g, bl, a, a.contrast_at, 0.0f);
    acc = acc + aug_gray(r, g, bl);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)b * AUG_GROUPS + k] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}
__global__ __launch_bounds__(256) void aug_gray_mean_kernel(const uint8_t* __restrict__ img, long n_split, int Hs, int Ws,
                                                            const int64_t* __restrict__ rows, const int* __restrict__ boxes,
                                                            const int* __restrict__ aug, float* __restrict__ partial, int B, int C,
                                                            int Hi, int Wi) {
  aug_gray_mean<false>(img, n_split, Hs, Ws, rows, boxes, aug, nullptr, nullptr, partial, B, C, Hi, Wi);
}
__global__ __launch_bounds__(256) void aug_gray_mean_ra_kernel(const uint8_t* __restrict__ img, long n_split, int Hs, int Ws,
                                                               const int64_t* __restrict__ rows, const int* __restrict__ boxes,
                                                               const int* __restrict__ aug, const int* __restrict__ ra,
                                                               const uint8_t* __restrict__ lut, float* __restrict__ partial, int B, int C,
                                                               int Hi, int Wi) {
  aug_gray_mean<true>(img, n_split, Hs, Ws, rows, boxes, aug, ra, lut, partial, B, C, Hi, Wi);
}
__global__ __launch_bounds__(64) void aug_gray_mean_reduce_kernel(const int* __restrict__ aug, const float* __restrict__ partial,
                                                                  float* __restrict__ stat, int B, int Hi, int Wi) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  AugRow a;
  if (!aug_row(aug, b, Hi, Wi, &a) || a.contrast_at == 3) return;
  const float* p = partial + (size_t)b * AUG_GROUPS;
  float t = p[0];
  for (int k = 1; k < AUG_GROUPS; ++k) t = t + p[k];
  stat[b] = t / (float)(Hi * Wi);
}

// What one lane of either body writes: the four elements from `e` of the output, which are channel c, output pixels (oy, ox ..
// ox + 3) of sample b.  Output row b per + j is patch pr of sample b: dense rows, per = gh gw and pr = j; KEEP (patch dropout,
// keep int32 [B,K]), per = K and pr = keep[b][j] -- from pr on the text is the same, so a kept row is bit for bit the row of the
// same patch.  sample_ok(b) is the body's check of everything sample b reads, made before keep[b][j] is read.  A sample it refuses
// is never dereferenced: its rows are zeros and the lane of its first element counts it once in *bad (may be NULL); otherwise a
// keep entry outside [0, gh gw) is never used: a zero row, counted by the lane of that row's first element.  false: this lane has
// written its zeros.  sample_ok is called exactly once, before anything else of the sample is used: a body may leave what it read of
// the sample (its image index, its table rows) in variables of its own from there, valid where feed_lane returns true.
struct FeedLane { long e; int b, c, oy, ox; };
template <bool KEEP, class SampleOk>
__device__ __forceinline__ bool feed_lane(const cara_feed& f, bf16* __restrict__ out, long idx, SampleOk&& sample_ok, FeedLane* L) {
  const int p = f.p, gw = f.Wi / p, gh = f.Hi / p;
  const int kcols = f.C * p * p;
  const long e = idx * 4;
  const long row = e / kcols;
  const int col = (int)(e - row * kcols);
  const int c = col / (p * p), py = (col / p) % p, px = col % p;
  const int per = KEEP ? f.K : gh * gw;
  const int b = (int)(row / per), j = (int)(row % per);
  int pr = j;
  bool ok = sample_ok(b), counts = j == 0 && col == 0;
  if (KEEP && ok) {
    pr = f.keep[(size_t)b * f.K + j];
    ok = pr >= 0 && pr < gh * gw;
    counts = col == 0;
  }
  if (!ok) {
    if (f.bad && counts) atomicAdd(f.bad, 1);
    const bf16 z = (bf16)0.0f;
    *reinterpret_cast<bf16x4*>(out + e) = bf16x4{z, z, z, z};
    return false;
  }
  const int gy = pr / gw, gx = pr % gw;
  *L = FeedLane{e, b, c, gy * p + py, gx * p + px};
  return true;
}

// The aligned body: T = float, images fp32 [B,C,Hi,Wi] -> one float4 per lane (p % 4 == 0: a 16-float image row segment per 4
// lanes); T = uint8_t, pixels [.,C,Hi,Wi] -> one dword per lane through normalize_u8x4.  Sample b is image b of the batch, or with
// `rows` image rows[b] of a whole resident split of n_split (any order, duplicates allowed); an index outside [0, n_split) is refused.
template <class T, bool KEEP>
__global__ __launch_bounds__(256) void aligned_rows_kernel(const cara_feed f, bf16* __restrict__ out, long total4) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // four elements of a patch row
  if (idx >= total4) return;
  FeedLane L;
  int64_t r;   // (set by the check below, which feed_lane calls once)
  if (!feed_lane<KEEP>(f, out, idx, [&](int b) {
        // (an fp32 source is a batch: the validator refuses `rows` beside `images`, and the float forms do not carry the branch)
        const bool split = !std::is_same<T, float>::value && f.rows;
        r = split ? f.rows[b] : b;
        return !split || (r >= 0 && r < f.n_split);
      }, &L))
    return;
  const size_t at = (((size_t)r * f.C + L.c) * f.Hi + L.oy) * f.Wi + L.ox;
  if constexpr (std::is_same<T, float>::value) {
    const float4 v = *reinterpret_cast<const float4*>(f.images + at);
    bf16x4 o = {(bf16)v.x, (bf16)v.y, (bf16)v.z, (bf16)v.w};
    *reinterpret_cast<bf16x4*>(out + L.e) = o;
  } else {
    const unsigned u = *reinterpret_cast<const unsigned*>(f.pixels + at);
    *reinterpret_cast<bf16x4*>(out + L.e) = normalize_u8x4(u, f.mean[L.c], f.stdv[L.c]);
  }
}

// The box body.  MIX: a mix table may be present; AUG: an aug table is (and a mix table may be); RA: an ra table is (and the other
// two may be).  What a sample is checked for and carries follows from AUG and RA: its source, its jitter row and its ra row.
struct NoRow {};
template <bool AUG, bool RA>
struct FeedSample { MixSource box; std::conditional_t<AUG, AugRow, NoRow> a; std::conditional_t<RA, RaRow, NoRow> r; };
template <bool AUG, bool RA>
__device__ __forceinline__ bool feed_sample(const cara_feed& f, int b, FeedSample<AUG, RA>* s) {
  if (!mix_source(f.pixels, f.n_split, f.C, f.Hs, f.Ws, f.rows, f.boxes, b, &s->box)) return false;
  if constexpr (RA) {
    if (!ra_row(f.ra, b, &s->r)) return false;
  }
  if constexpr (AUG) return aug_row(f.aug, b, f.Hi, f.Wi, &s->a);
  else return true;
}
// channel c of output pixel (ox, oy) of a sample, un-normalised and unmixed; lut: the sample's ra tables (RA alone)
template <bool AUG, bool RA>
__device__ __forceinline__ float feed_value(const cara_feed& f, const RowSource& s, const FeedSample<AUG, RA>& smp, const uint8_t* lut, float M,
                                            int c, int ox, int oy) {
  const CropAxis ax = crop_axis(ox, f.Wi, s.w, s.flip);
  auto crop = [&](int ch) { return crop_value(s.top + ch * s.plane, s.bot + ch * s.plane, ax, s.fy); };
  auto base = [&](int ch) {
    if constexpr (RA) return ra_value(smp.box, smp.r, lut, ch, ox, oy, f.Hi, f.Wi, f.Ws, s.plane, 3, crop);
    else return crop(ch);
  };
  if constexpr (AUG) return aug_value(base, smp.a, M, c);
  else return base(c);
}
// A lane keeps four adjacent output pixels of one channel of one patch row (the row pair and fy are shared).  A sample is refused
// -- zeros, counted once -- where its own or its partner's row, box, jitter row or ra row is bad, its partner is outside [0, B)
// (checked before anything of the partner's is formed), its rectangle is not inside the output or its m is not in [0, 1].
template <bool MIX, bool AUG, bool RA, bool KEEP>
__device__ __forceinline__ void box_rows(const cara_feed& f, bf16* __restrict__ out, long total4) {
  static_assert(MIX || !(AUG || RA), "the jitter and ra forms are the mix form's extensions");
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total4) return;
  const int Hi = f.Hi, Wi = f.Wi;
  FeedLane L;
  MixRow mr;                       // (these three are set by the check below, which feed_lane calls once; oth only where the
  FeedSample<AUG, RA> own, oth;    // sample has a partner that is not itself)
  if (!feed_lane<KEEP>(f, out, idx, [&](int b) {
        mr = mix_row<MIX, AUG || RA>(f.mix, b);
        // (each sample's jitter and ra rows are checked beside its source; a sample that is its own partner checks one source)
        return feed_sample(f, b, &own) &&
               (mr.partner == b || (mr.partner >= 0 && mr.partner < f.B && feed_sample(f, mr.partner, &oth))) && mix_row_ok(mr, Hi, Wi);
      }, &L))
    return;
  const int b = L.b, c = L.c, oy = L.oy;
  if (MIX && mr.partner == b) oth = own;
  const RowSource s_own = row_source(own.box, oy, Hi, f.Hs, f.Ws), s_oth = MIX ? row_source(oth.box, oy, Hi, f.Hs, f.Ws) : s_own;
  float M_own = 0.0f, M_oth = 0.0f;
  bool erow_in = false;
  unsigned i0 = 0;
  if constexpr (AUG) {
    // (a statistic is read only where its sample has a contrast slot: the pre-pass wrote exactly those)
    const float* stat = static_cast<const float*>(f.stat);
    M_own = own.a.contrast_at < 3 ? stat[b] : 0.0f;
    M_oth = oth.a.contrast_at < 3 ? stat[mr.partner] : 0.0f;
    erow_in = oy >= own.a.ey0 && oy - own.a.ey0 < own.a.eh;
    i0 = (((unsigned)b * (unsigned)f.C + (unsigned)c) * (unsigned)Hi + (unsigned)oy) * (unsigned)Wi + (unsigned)L.ox;
  }
  // (a table is read only at a statistic slot: ra_table_kernel wrote exactly those samples')
  const uint8_t *lut_own = nullptr, *lut_oth = nullptr;
  if constexpr (RA) {
    lut_own = static_cast<const uint8_t*>(f.ra_stat) + (size_t)b * (3 * 256);
    lut_oth = static_cast<const uint8_t*>(f.ra_stat) + (size_t)mr.partner * (3 * 256);
  }
  const bool row_in = oy >= mr.cy0 && oy - mr.cy0 < mr.ch;
  const float mu = f.mean[c], sd = f.stdv[c];
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = L.ox + j;
    float a;
    if constexpr (!MIX) {
      a = feed_value(f, s_own, own, lut_own, M_own, c, ox, oy);
    } else if (row_in && ox >= mr.cx0 && ox - mr.cx0 < mr.cw) {
      a = feed_value(f, s_oth, oth, lut_oth, M_oth, c, ox, oy);
    } else {
      a = feed_value(f, s_own, own, lut_own, M_own, c, ox, oy);
      if (mr.m != 0.0f) a = mix_blend(a, mr.m, feed_value(f, s_oth, oth, lut_oth, M_oth, c, ox, oy));
    }
    v[j] = normalize_f32(a, mu, sd);
    if constexpr (AUG) {
      if (erow_in && ox >= own.a.ex0 && ox - own.a.ex0 < own.a.ew) v[j] = own.a.emode ? aug_noise(i0 + (unsigned)j, own.a.eseed) : 0.0f;
    }
  }
  *reinterpret_cast<bf16x4*>(out + L.e) = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
template <bool MIX, bool AUG, bool KEEP>
__global__ __launch_bounds__(256) void box_rows_kernel(const cara_feed f, bf16* __restrict__ out, long total4) {
  box_rows<MIX, AUG, false, KEEP>(f, out, total4);
}
template <bool AUG, bool KEEP>
__global__ __launch_bounds__(256) void box_rows_ra_kernel(const cara_feed f, bf16* __restrict__ out, long total4) {
  box_rows<true, AUG, true, KEEP>(f, out, total4);
}

// out[i] = labels[rows[i]]; a row outside [0, n_split) is not dereferenced: it gives 0 and is counted in *bad (may be NULL)
__global__ __launch_bounds__(256) void gather_labels_kernel(const int64_t* __restrict__ labels, long n_split,
                                                            const int64_t* __restrict__ rows, int64_t* __restrict__ out,
                                                            int B, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int64_t r = rows[i];
  const bool ok = r >= 0 && r < n_split;
  if (!ok && bad) atomicAdd(bad, 1);
  out[i] = ok ? labels[r] : 0;
}

// the instantiation a descriptor asks for: the plainest body that has every table it sets
using FeedKernel = void (*)(cara_feed, bf16*, long);
template <bool KEEP>
FeedKernel feed_kernel(const cara_feed& f) {
  if (f.ra) return f.aug ? box_rows_ra_kernel<true, KEEP> : box_rows_ra_kernel<false, KEEP>;
  if (f.aug) return box_rows_kernel<true, true, KEEP>;
  if (f.mix) return box_rows_kernel<true, false, KEEP>;
  if (f.boxes) return box_rows_kernel<false, false, KEEP>;
  if (f.images) return aligned_rows_kernel<float, KEEP>;
  return aligned_rows_kernel<uint8_t, KEEP>;
}

// a call without source size or tables: whole images of the output's size
cara_feed whole_images(int B, int C, int Hi, int Wi, int p) {
  cara_feed f = {};
  f.Hs = Hi; f.Ws = Wi;
  f.B = B; f.C = C; f.Hi = Hi; f.Wi = Wi; f.p = p;
  return f;
}

}  // namespace

int cara_feed_patch_rows(const cara_feed& f, void* patches, void* stream) {
  if (!patches || f.B <= 0 || f.C <= 0 || f.p <= 0 || (f.p & 3) || f.Hi <= 0 || f.Wi <= 0 || f.Hi % f.p || f.Wi % f.p) return CARA_E_ARG;
  if (f.Hs <= 0 || f.Ws <= 0) return CARA_E_ARG;
  if (!f.boxes && (f.Hs != f.Hi || f.Ws != f.Wi)) return CARA_E_ARG;   // (without boxes a sample is its whole image, byte for byte)
  const int grid_rows = (f.Hi / f.p) * (f.Wi / f.p);
  if (f.keep && (f.K < 1 || f.K > grid_rows)) return CARA_E_ARG;
  const bool box = f.boxes || f.mix || f.aug || f.ra;
  if (f.images) {
    if (f.pixels || f.rows || box) return CARA_E_ARG;
  } else {
    if (!f.pixels || !f.mean || !f.stdv) return CARA_E_ARG;
    if (f.rows ? f.n_split <= 0 : box) return CARA_E_ARG;   // (boxes and tables are per row of a split)
  }
  // (dword loads: with p % 4 == 0 and Wi % 4 == 0 every image, row and patch segment starts dword-aligned)
  if (!box && ((f.Wi & 3) || (reinterpret_cast<uintptr_t>(f.pixels) & 3))) return CARA_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint8_t* lut = static_cast<uint8_t*>(f.ra_stat);
  // (every refusal before the first launch)
  if (f.ra && (f.C != 3 || !f.ra_stat || (reinterpret_cast<uintptr_t>(f.ra_stat) & 3))) return CARA_E_ARG;   // (fill is three bytes, the tables per channel of three)
  if (f.aug) {
    if (f.C != 3) return CARA_E_ARG;                              // (the colour ops are defined on three channels)
    if (!f.stat || (reinterpret_cast<uintptr_t>(f.stat) & 3)) return CARA_E_ARG;
    if (2ull * (unsigned long long)f.B * f.C * f.Hi * f.Wi > (1ull << 32)) return CARA_E_ARG;   // (the noise's two counters per element are 32-bit)
  }
  if (f.ra) {
    int* partial = reinterpret_cast<int*>(lut + (size_t)f.B * (3 * 256));
    hipLaunchKernelGGL(ra_hist_kernel, dim3((unsigned)f.B * RA_GROUPS), dim3(256), 0, st, f.pixels, (long)f.n_split, f.Hs, f.Ws, f.rows, f.boxes,
                       f.ra, partial, f.B, f.C, f.Hi, f.Wi);
    CARA_CHECK_LAUNCH();
    hipLaunchKernelGGL(ra_table_kernel, dim3((unsigned)f.B * 3), dim3(256), 0, st, f.ra, partial, lut, f.B);
    CARA_CHECK_LAUNCH();
  }
  if (f.aug) {
    float* stat = static_cast<float*>(f.stat);
    float* partial = stat + f.B;
    if (f.ra)
      hipLaunchKernelGGL(aug_gray_mean_ra_kernel, dim3((unsigned)f.B * AUG_GROUPS), dim3(256), 0, st, f.pixels, (long)f.n_split, f.Hs, f.Ws,
                         f.rows, f.boxes, f.aug, f.ra, lut, partial, f.B, f.C, f.Hi, f.Wi);
    else
      hipLaunchKernelGGL(aug_gray_mean_kernel, dim3((unsigned)f.B * AUG_GROUPS), dim3(256), 0, st, f.pixels, (long)f.n_split, f.Hs, f.Ws, f.rows,
                         f.boxes, f.aug, partial, f.B, f.C, f.Hi, f.Wi);
    CARA_CHECK_LAUNCH();
    hipLaunchKernelGGL(aug_gray_mean_reduce_kernel, dim3((unsigned)((f.B + 63) / 64)), dim3(64), 0, st, f.aug, partial, stat, f.B, f.Hi, f.Wi);
    CARA_CHECK_LAUNCH();
  }
  const long total4 = (long)f.B * (f.keep ? f.K : grid_rows) * f.C * f.p * f.p / 4;
  const FeedKernel kernel = f.keep ? feed_kernel<true>(f) : feed_kernel<false>(f);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, f, (bf16*)patches, total4);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}

extern "C" int cara_im2col_patches(const float* img, void* patches, int B, int C, int Hi, int Wi, int p, void* stream) {
  if (!img) return CARA_E_ARG;
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.images = img;
  return cara_feed_patch_rows(f, patches, stream);
}

extern "C" int cara_im2col_patches_u8(const unsigned char* pixels, const float* mean, const float* stdv, void* patches, int B, int C,
                                      int Hi, int Wi, int p, void* stream) {
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.pixels = pixels; f.mean = mean; f.stdv = stdv;
  return cara_feed_patch_rows(f, patches, stream);
}

extern "C" int cara_im2col_patches_u8_rows(const unsigned char* pixels, int n_split, const int64_t* rows, const float* mean,
                                           const float* stdv, void* patches, int* bad, int B, int C, int Hi, int Wi, int p,
                                           void* stream) {
  if (!rows) return CARA_E_ARG;
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.pixels = pixels; f.mean = mean; f.stdv = stdv; f.n_split = n_split; f.rows = rows; f.bad = bad;
  return cara_feed_patch_rows(f, patches, stream);
}

// no table: the launches of the call without one
extern "C" int cara_im2col_patches_u8_rows_aug(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                               const int* boxes, const int* mix, const int* aug, void* stat_scratch, const float* mean,
                                               const float* stdv, void* patches, int* bad, int B, int C, int Hi, int Wi, int p,
                                               void* stream) {
  if (!rows) return CARA_E_ARG;
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.pixels = pixels; f.mean = mean; f.stdv = stdv; f.n_split = n_split; f.rows = rows; f.bad = bad;
  f.Hs = Hs; f.Ws = Ws; f.boxes = boxes; f.mix = mix; f.aug = aug; f.stat = stat_scratch;
  return cara_feed_patch_rows(f, patches, stream);
}

extern "C" int cara_im2col_patches_u8_rows_crop(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                                const int* boxes, const float* mean, const float* stdv, void* patches, int* bad,
                                                int B, int C, int Hi, int Wi, int p, void* stream) {
  if (!boxes) return CARA_E_ARG;
  return cara_im2col_patches_u8_rows_aug(pixels, n_split, Hs, Ws, rows, boxes, nullptr, nullptr, nullptr, mean, stdv, patches, bad, B, C, Hi, Wi,
                                         p, stream);
}

extern "C" int cara_im2col_patches_u8_rows_mix(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                               const int* boxes, const int* mix, const float* mean, const float* stdv, void* patches,
                                               int* bad, int B, int C, int Hi, int Wi, int p, void* stream) {
  if (!mix) return CARA_E_ARG;
  return cara_im2col_patches_u8_rows_aug(pixels, n_split, Hs, Ws, rows, boxes, mix, nullptr, nullptr, mean, stdv, patches, bad, B, C, Hi, Wi, p,
                                         stream);
}

extern "C" size_t cara_aug_stat_bytes(int B) { return B > 0 ? (size_t)B * (1 + AUG_GROUPS) * sizeof(float) : 0; }

// Patch dropout: the entries above on a kept subset (keep int32 [B,K], 1 <= K <= gh gw).  B K rows are written, nothing beyond.
extern "C" int cara_im2col_patches_keep(const float* img, const int* keep, int K, void* patches, int* bad, int B, int C, int Hi, int Wi,
                                        int p, void* stream) {
  if (!img || !keep) return CARA_E_ARG;
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.images = img; f.bad = bad; f.keep = keep; f.K = K;
  return cara_feed_patch_rows(f, patches, stream);
}

extern "C" int cara_im2col_patches_u8_rows_keep(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                                const int* boxes, const int* mix, const int* aug, void* stat_scratch, const int* keep,
                                                int K, const float* mean, const float* stdv, void* patches, int* bad, int B, int C,
                                                int Hi, int Wi, int p, void* stream) {
  if (!rows || !keep) return CARA_E_ARG;
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.pixels = pixels; f.mean = mean; f.stdv = stdv; f.n_split = n_split; f.rows = rows; f.bad = bad;
  f.Hs = Hs; f.Ws = Ws; f.boxes = boxes; f.mix = mix; f.aug = aug; f.stat = stat_scratch; f.keep = keep; f.K = K;
  return cara_feed_patch_rows(f, patches, stream);
}

// RandAugment by index: every table but `rows` may be NULL; without `ra` the launches of the _keep / _aug entries
extern "C" int cara_im2col_patches_u8_rows_ra(const unsigned char* pixels, int n_split, int Hs, int Ws, const int64_t* rows,
                                              const int* boxes, const int* mix, const int* aug, void* stat_scratch, const int* ra,
                                              void* ra_scratch, const int* keep, int K, const float* mean, const float* stdv,
                                              void* patches, int* bad, int B, int C, int Hi, int Wi, int p, void* stream) {
  if (!rows) return CARA_E_ARG;
  cara_feed f = whole_images(B, C, Hi, Wi, p);
  f.pixels = pixels; f.mean = mean; f.stdv = stdv; f.n_split = n_split; f.rows = rows; f.bad = bad;
  f.Hs = Hs; f.Ws = Ws; f.boxes = boxes; f.mix = mix; f.aug = aug; f.stat = stat_scratch; f.ra = ra; f.ra_stat = ra_scratch;
  f.keep = keep; f.K = keep ? K : 0;
  return cara_feed_patch_rows(f, patches, stream);
}

extern "C" size_t cara_ra_stat_bytes(int B) { return B > 0 ? (size_t)B * (3 * 256) * (1 + RA_GROUPS * sizeof(int)) : 0; }

extern "C" int cara_gather_labels(const int64_t* labels, int n_split, const int64_t* rows, int64_t* out, int B, int* bad,
                                  void* stream) {
  if (!labels || !rows || !out || n_split <= 0 || B <= 0) return CARA_E_ARG;
  hipLaunchKernelGGL(gather_labels_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     labels, (long)n_split, rows, out, B, bad);
  CARA_CHECK_LAUNCH();
  return CARA_OK;
}
