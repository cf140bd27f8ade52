// Per-model masked forms of the flat-buffer ops (per-model early
// stopping):
//   optimizer_step_masked  every optimizer kind of adam_kernel /
//                          opt_kernel<KIND>, skipping the models whose
//                          active[g] == 0
//   masked_copy            dst <- src (+ bf16 mirror) for the models
//                          whose mask[g] != 0
//   remap_models           whole models from a [G_src, ...] buffer into
//                          a [G_dst, ...] buffer (+ bf16 mirror), by a
//                          list of (dst model, src model) pairs: pack
//                          compaction (see remap_models_kernel)
//   optimizer_step_reg     the masked step with the weight regularizers'
//                          gradient term l1 sgn(w) + 2 l2 w fused at the
//                          gradient load, per tensor (opt_masked_kernel
//                          <KIND, true>; the mask is optional)
//   weight_penalty         per-model sum of l1 sum|w| + l2 sum w^2 over
//                          the tensors (weight_penalty_*_kernel)
//
// The flat buffer holds S declared tensors; tensor s is [G, per_s], so
// model g owns [off_s + g*per_s, off_s + (g+1)*per_s). The segment
// table is a device int64 [2, S] array: row 0 the offsets, row 1 the
// per-model sizes.
//
// Layout: grid (chunks, G), 256 threads. Block (c, g) reads active[g]
// once and returns as a whole when it is 0 (a block-uniform branch: no
// load or store of a frozen model is ever issued). Otherwise the
// `chunks` blocks of model g share the model's work units of 1024
// elements (256 lanes x 4): segment s is ceil(per_s / 1024) units, the
// units of all segments are numbered consecutively, and lane t < S of
// a block reads segment t's table entry and counts the units before it
// (walk_model_units: one round of table loads per block, S <= 256, no
// per-element division or search). Inside a unit consecutive lanes sit
// on consecutive addresses. A segment moves as 16-byte float4 (8-byte
// bf16x4 for the mirror) when per_s % 4 == 0, its base off_s + g*per_s
// is a multiple of 4 and every buffer is 16-byte aligned (the pad8
// layout); it moves element-wise otherwise. The host sizes `chunks`
// from n / G and S alone (it never reads the table), normally to one
// unit per block. A table entry that does not fit into the buffer is
// skipped, so a bad table cannot make the kernel touch memory outside
// it.
//
// The per-element expressions repeat those of adam_kernel
// (gordo_kernels.hip) and opt_kernel<KIND> (train_ops.hip), so an
// active model's result is bit-equal to the unmasked step (see the
// note at the RMSprop arm).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <tuple>
#include <vector>

namespace {

#define MK_DEV_INLINE __device__ __forceinline__

using bf16 = __hip_bfloat16;

// optimizer codes: 0 is plain Adam (adam_kernel), 1..5 those of
// train_ops.hip
constexpr int OPT_ADAM = 0, OPT_SGD = 1, OPT_RMSPROP = 2, OPT_ADAGRAD = 3,
              OPT_ADAM_AMSGRAD = 4, OPT_ADAMAX = 5;

struct OptConsts {
  float h0, h1, h2, h3;  // plain Adam: lr, beta1, beta2, eps
  float bc1, bc2;
  int flag;
};

MK_DEV_INLINE bf16 f2bf(float v) { return __float2bfloat16(v); }

// one element of the step: gi the gradient, pi the parameter, a/b/c the
// state slots 0/1/2 (read and written only where the kind uses them)
template <int KIND>
MK_DEV_INLINE void opt_elem(const OptConsts& k, float gi, float& pi, float& a,
                            float& b, float& c) {
  const float h0 = k.h0, h1 = k.h1, h2 = k.h2, h3 = k.h3;
  const float bc1 = k.bc1, bc2 = k.bc2;
  if (KIND == OPT_ADAM) {
    const float lr = h0, b1 = h1, b2 = h2, eps = h3;
    float mi = b1 * a + (1.f - b1) * gi;
    float vi = b2 * b + (1.f - b2) * gi * gi;
    a = mi;
    b = vi;
    pi = pi - lr / bc1 * mi / (sqrtf(vi / bc2) + eps);
  } else if (KIND == OPT_SGD) {
    if (h1 == 0.f) {
      pi -= h0 * gi;
    } else {
      float mi = h1 * a - h0 * gi;
      a = mi;
      pi += k.flag ? h1 * mi - h0 * gi : mi;
    }
  } else if (KIND == OPT_RMSPROP) {
    // opt_kernel<OPT_RMSPROP> forms this sum from rounded products
    // (its two multiplies pair up as one packed multiply, which leaves
    // no multiply-add to fuse); fusing here would differ in the last
    // bit, so contraction is off for this one statement
    float vi;
    {
#pragma clang fp contract(off)
      vi = h1 * a + (1.f - h1) * gi * gi;
    }
    a = vi;
    float inc = h0 * gi / sqrtf(vi + h3);
    if (h2 > 0.f) {
      float mi = h2 * b + inc;
      b = mi;
      pi -= mi;
    } else {
      pi -= inc;
    }
  } else if (KIND == OPT_ADAGRAD) {
    float ai = a + gi * gi;
    a = ai;
    pi -= h0 * gi / sqrtf(ai + h1);
  } else if (KIND == OPT_ADAM_AMSGRAD) {
    float mi = h1 * a + (1.f - h1) * gi;
    float vi = h2 * b + (1.f - h2) * gi * gi;
    float vh = fmaxf(c, vi);
    a = mi;
    b = vi;
    c = vh;
    pi -= h0 * sqrtf(bc2) / bc1 * mi / (sqrtf(vh) + h3);
  } else {  // OPT_ADAMAX
    float mi = h1 * a + (1.f - h1) * gi;
    float ui = fmaxf(h2 * b, fabsf(gi));
    a = mi;
    b = ui;
    pi -= h0 / bc1 * mi / (ui + h3);
  }
}

MK_DEV_INLINE void store_bf16x4(bf16* dst, const float4& v) {
  union {
    bf16 h[4];
    uint2 u;
  } pk;
  pk.h[0] = f2bf(v.x);
  pk.h[1] = f2bf(v.y);
  pk.h[2] = f2bf(v.z);
  pk.h[3] = f2bf(v.w);
  *reinterpret_cast<uint2*>(dst) = pk.u;
}

// the segment's slice of model g, or false when the table entry does
// not fit into the n-element buffer
MK_DEV_INLINE bool segment_slice(const long long* __restrict__ table, int S,
                                 int s, int g, int G, size_t n,
                                 size_t n_model, size_t& base, size_t& per) {
  long long off = table[s];
  long long len = table[S + s];
  if (off < 0 || len <= 0) return false;
  // n_model = n / G (from the host), so len * G cannot exceed n
  if ((size_t)len > n_model || (size_t)off > n - (size_t)len * G)
    return false;
  base = (size_t)off + (size_t)g * (size_t)len;
  per = (size_t)len;
  return true;
}

// A block moves UNIT elements at a time: 256 lanes x 4 elements.
constexpr int UNIT_SHIFT = 10;
constexpr size_t UNIT = (size_t)1 << UNIT_SHIFT;
// one lane per segment builds the unit table: S <= block size
constexpr int MAX_SEGMENTS = 256;

// Walks model g's work units for block blockIdx.x of gridDim.x (256
// threads, all of them must call it). A segment of per_s elements is
// ceil(per_s / UNIT) units, and the units of the S segments are
// numbered one after the other. Lane t < S reads segment t's table
// entry and counts the units before it (LDS, 4 arrays of S words); the
// block then takes units blockIdx.x, blockIdx.x + gridDim.x, ...: the
// one lane whose segment holds the unit names it, no division and no
// search. For unit u it calls unit(s, base, per, lo, hi, u) in every
// thread, with block-uniform arguments: the segment's index, the flat
// index of its slice of model g, its per-model size and the unit's
// element range [lo, hi) of the slice. The numbering depends on the
// per_s alone, not on G or on the grid.
template <class FU>
MK_DEV_INLINE void walk_units(const long long* __restrict__ table, int S,
                              int g, int G, size_t n, size_t n_model,
                              FU&& unit) {
  // lane t < S holds segment t: one round of table loads for the whole
  // block instead of a chain of dependent scalar loads per segment
  __shared__ size_t sh_base[MAX_SEGMENTS], sh_per[MAX_SEGMENTS];
  __shared__ size_t sh_units[MAX_SEGMENTS], sh_first[MAX_SEGMENTS];
  __shared__ size_t sh_total;
  __shared__ int sh_seg;
  const int t = threadIdx.x;
  size_t my_units = 0;
  if (t < S) {
    size_t base = 0, per = 0;
    if (segment_slice(table, S, t, g, G, n, n_model, base, per))
      my_units = (per + UNIT - 1) >> UNIT_SHIFT;
    sh_base[t] = base;
    sh_per[t] = per;
    sh_units[t] = my_units;
  }
  __syncthreads();
  // number of segment t's first unit: the units of the segments before
  size_t my_first = 0;
  if (t < S) {
    for (int j = 0; j < t; ++j) my_first += sh_units[j];
    sh_first[t] = my_first;
    if (t == S - 1) sh_total = my_first + my_units;
  }
  __syncthreads();
  const size_t total = sh_total;
  // the trip count depends on blockIdx and total alone: uniform
  for (size_t u = blockIdx.x; u < total; u += gridDim.x) {
    if (t < S && u >= my_first && u < my_first + my_units) sh_seg = t;
    __syncthreads();
    const int s = sh_seg;
    const size_t base = sh_base[s], per = sh_per[s];
    const size_t first = sh_first[s];
    __syncthreads();  // sh_seg is read: the next round may write it
    const size_t lo = (u - first) << UNIT_SHIFT;
    const size_t hi = lo + UNIT < per ? lo + UNIT : per;
    unit(s, base, per, lo, hi, u);
  }
}

// The elements [lo, hi) of one unit: per lane, vec4(e) for 4 elements
// at flat index e where the segment moves as 16-byte vectors, else
// one(e) per element with the block's lanes on consecutive e.
template <class FV, class FS>
MK_DEV_INLINE void unit_elems(size_t base, size_t per, size_t lo, size_t hi,
                              int vec_ok, FV&& vec4, FS&& one) {
  if (vec_ok && (per & 3) == 0 && (base & 3) == 0) {
    const size_t i = lo + ((size_t)threadIdx.x << 2);
    if (i < hi) vec4(base + i);  // hi % 4 == 0: the 4 are inside
  } else {
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
      one(base + i);
  }
}

// walk_units with every unit moved by unit_elems
template <class FV, class FS>
MK_DEV_INLINE void walk_model_units(const long long* __restrict__ table,
                                    int S, int g, int G, size_t n,
                                    size_t n_model, int vec_ok, FV&& vec4,
                                    FS&& one) {
  walk_units(table, S, g, G, n, n_model,
             [&](int, size_t base, size_t per, size_t lo, size_t hi, size_t) {
               unit_elems(base, per, lo, hi, vec_ok, vec4, one);
             });
}

// The weight regularizer's share of the gradient: a tensor with
// coefficients (l1, l2) adds l1 sum|w| + l2 sum w^2 to its model's loss,
// so the optimizer sees gi + (l1 sgn(pi) + (2 l2) pi), sgn(+-0) = 0: a
// zero-padded entry with a zero gradient stays exactly zero. Products
// and sums are rounded one by one (no contraction): ops/reference.py
// repeats this expression.
MK_DEV_INLINE float reg_grad(float gi, float pi, float l1, float l2x2) {
#pragma clang fp contract(off)
  const float sgn = (float)(pi > 0.f) - (float)(pi < 0.f);
  const float t1 = l1 * sgn;
  const float t2 = l2x2 * pi;
  const float r = t1 + t2;
  return gi + r;
}

struct StepBufs {
  float* __restrict__ p;
  const float* __restrict__ g;
  float* __restrict__ s0;
  float* __restrict__ s1;
  float* __restrict__ s2;
  bf16* __restrict__ plp;
  bool use0, use1, use2;
};

// 4 elements at flat index e; R: with the regularizer term
template <int KIND, bool R>
MK_DEV_INLINE void step_vec4(const StepBufs& m, const OptConsts& k, size_t e,
                             float l1, float l2x2) {
  float4 gv = *reinterpret_cast<const float4*>(m.g + e);
  float4 pv = *reinterpret_cast<const float4*>(m.p + e);
  float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av, cv = av;
  if (m.use0) av = *reinterpret_cast<const float4*>(m.s0 + e);
  if (m.use1) bv = *reinterpret_cast<const float4*>(m.s1 + e);
  if (m.use2) cv = *reinterpret_cast<const float4*>(m.s2 + e);
  if (R) {
    gv.x = reg_grad(gv.x, pv.x, l1, l2x2);
    gv.y = reg_grad(gv.y, pv.y, l1, l2x2);
    gv.z = reg_grad(gv.z, pv.z, l1, l2x2);
    gv.w = reg_grad(gv.w, pv.w, l1, l2x2);
  }
  opt_elem<KIND>(k, gv.x, pv.x, av.x, bv.x, cv.x);
  opt_elem<KIND>(k, gv.y, pv.y, av.y, bv.y, cv.y);
  opt_elem<KIND>(k, gv.z, pv.z, av.z, bv.z, cv.z);
  opt_elem<KIND>(k, gv.w, pv.w, av.w, bv.w, cv.w);
  if (m.use0) *reinterpret_cast<float4*>(m.s0 + e) = av;
  if (m.use1) *reinterpret_cast<float4*>(m.s1 + e) = bv;
  if (m.use2) *reinterpret_cast<float4*>(m.s2 + e) = cv;
  *reinterpret_cast<float4*>(m.p + e) = pv;
  if (m.plp) store_bf16x4(m.plp + e, pv);
}

template <int KIND, bool R>
MK_DEV_INLINE void step_one(const StepBufs& m, const OptConsts& k, size_t e,
                            float l1, float l2x2) {
  float gi = m.g[e];
  float pi = m.p[e];
  float a = 0.f, b = 0.f, c = 0.f;
  if (m.use0) a = m.s0[e];
  if (m.use1) b = m.s1[e];
  if (m.use2) c = m.s2[e];
  if (R) gi = reg_grad(gi, pi, l1, l2x2);
  opt_elem<KIND>(k, gi, pi, a, b, c);
  if (m.use0) m.s0[e] = a;
  if (m.use1) m.s1[e] = b;
  if (m.use2) m.s2[e] = c;
  m.p[e] = pi;
  if (m.plp) m.plp[e] = f2bf(pi);
}

// REG: `reg` is the float [2, S] coefficient table beside `table` (row
// 0 the l1, row 1 the l2 of each tensor) and `active` may be null (no
// model is frozen). A unit whose segment has both coefficients zero
// takes the REG = false element code: a block-uniform choice, and the
// same arithmetic as the plain masked step.
template <int KIND, bool REG>
__global__ void opt_masked_kernel(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ s2,
    bf16* __restrict__ plp, size_t n, float h0, float h1, float h2, float h3,
    int flag, const int* __restrict__ step_buf,
    const int* __restrict__ active, const long long* __restrict__ table,
    int S, int vec_ok, size_t n_model, const float* __restrict__ reg) {
  const int mg = blockIdx.y;
  if (REG) {
    if (active != nullptr && active[mg] == 0) return;
  } else {
    if (active[mg] == 0) return;
  }
  OptConsts k;
  k.h0 = h0, k.h1 = h1, k.h2 = h2, k.h3 = h3;
  k.bc1 = 1.f, k.bc2 = 1.f;
  k.flag = flag;
  if (KIND == OPT_ADAM) {
    float fstep = (float)*step_buf;
    k.bc1 = 1.f - __powf(h1, fstep);
    k.bc2 = 1.f - __powf(h2, fstep);
  } else if (KIND == OPT_ADAM_AMSGRAD || KIND == OPT_ADAMAX) {
    float fstep = (float)*step_buf;
    k.bc1 = 1.f - powf(h1, fstep);
    k.bc2 = 1.f - powf(h2, fstep);
  }
  StepBufs m;
  m.p = p, m.g = g, m.s0 = s0, m.s1 = s1, m.s2 = s2, m.plp = plp;
  // which state slots this kind reads and writes (block-uniform)
  m.use0 = KIND != OPT_SGD || h1 != 0.f;
  m.use1 = KIND == OPT_ADAM || KIND == OPT_ADAM_AMSGRAD ||
           KIND == OPT_ADAMAX || (KIND == OPT_RMSPROP && h2 > 0.f);
  m.use2 = KIND == OPT_ADAM_AMSGRAD;
  walk_units(
      table, S, mg, (int)gridDim.y, n, n_model,
      [&](int s, size_t base, size_t per, size_t lo, size_t hi, size_t) {
        float l1 = 0.f, l2x2 = 0.f;
        if (REG) {
          l1 = reg[s];
          l2x2 = 2.f * reg[S + s];
        }
        if (REG && (l1 != 0.f || l2x2 != 0.f)) {
          unit_elems(
              base, per, lo, hi, vec_ok,
              [&](size_t e) { step_vec4<KIND, true>(m, k, e, l1, l2x2); },
              [&](size_t e) { step_one<KIND, true>(m, k, e, l1, l2x2); });
        } else {
          unit_elems(
              base, per, lo, hi, vec_ok,
              [&](size_t e) { step_vec4<KIND, false>(m, k, e, 0.f, 0.f); },
              [&](size_t e) { step_one<KIND, false>(m, k, e, 0.f, 0.f); });
        }
      });
}

// Per-model weight penalty, first pass: unit u of model g writes
// l1 sum|w| + l2 sum w^2 over its elements to part[g * U + u]. A
// model's bits must not depend on G, on its place in the pack or on
// the load form (a tensor that is 16-byte aligned in one layout is not
// in another, and compaction promises a bit-equal fit), so lane t
// always holds elements lo + 4t .. lo + 4t + 3 of the unit, loaded as
// one float4 or as four floats (0 past the end), and everything after
// the load is one piece of code: pairwise in the lane, a xor butterfly
// over the wave's 64 lanes, the 4 waves' sums pairwise through LDS. No
// atomics. A segment with both coefficients zero is not read: its
// units write 0.
__global__ void weight_penalty_units_kernel(
    const float* __restrict__ p, size_t n, const long long* __restrict__ table,
    const float* __restrict__ reg, int S, int vec_ok, size_t n_model,
    float* __restrict__ part, size_t U) {
  __shared__ float sh_a[4], sh_q[4];
  const int mg = blockIdx.y;
  const int t = threadIdx.x;
  walk_units(
      table, S, mg, (int)gridDim.y, n, n_model,
      [&](int s, size_t base, size_t per, size_t lo, size_t hi, size_t u) {
        const float l1 = reg[s], l2 = reg[S + s];
        float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
        if (l1 != 0.f || l2 != 0.f) {  // block-uniform
          const size_t i = lo + ((size_t)t << 2);
          if (vec_ok && (per & 3) == 0 && (base & 3) == 0) {
            if (i < hi) {  // hi % 4 == 0: the 4 are inside
              float4 v = *reinterpret_cast<const float4*>(p + base + i);
              x0 = v.x, x1 = v.y, x2 = v.z, x3 = v.w;
            }
          } else {
            if (i < hi) x0 = p[base + i];
            if (i + 1 < hi) x1 = p[base + i + 1];
            if (i + 2 < hi) x2 = p[base + i + 2];
            if (i + 3 < hi) x3 = p[base + i + 3];
          }
        }
        float a, q;
        {
#pragma clang fp contract(off)
          a = (fabsf(x0) + fabsf(x1)) + (fabsf(x2) + fabsf(x3));
          q = (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
        }
        for (int d = 32; d >= 1; d >>= 1) {
          a += __shfl_xor(a, d, 64);
          q += __shfl_xor(q, d, 64);
        }
        if ((t & 63) == 0) {
          sh_a[t >> 6] = a;
          sh_q[t >> 6] = q;
        }
        __syncthreads();
        if (t == 0 && u < U) {
#pragma clang fp contract(off)
          const float A = (sh_a[0] + sh_a[1]) + (sh_a[2] + sh_a[3]);
          const float Q = (sh_q[0] + sh_q[1]) + (sh_q[2] + sh_q[3]);
          const float ta = l1 * A;
          const float tq = l2 * Q;
          part[(size_t)mg * U + u] = ta + tq;
        }
        __syncthreads();  // sh_a / sh_q are read: the next unit writes
      });
}

// Second pass: one wave per model sums its units' partials, lane j
// units j, j + 64, ... in that order, then the same xor butterfly. The
// number of units follows from the per_s alone (counted as walk_units
// counts them), so the result does not depend on G or on the grid.
__global__ void weight_penalty_sum_kernel(
    const float* __restrict__ part, size_t U,
    const long long* __restrict__ table, int S, int G, size_t n,
    size_t n_model, float* __restrict__ out) {
  const int mg = blockIdx.x;
  const int t = threadIdx.x;  // 64 threads
  unsigned long long units = 0;
  for (int s = t; s < S; s += 64) {
    size_t base = 0, per = 0;
    if (segment_slice(table, S, s, mg, G, n, n_model, base, per))
      units += (per + UNIT - 1) >> UNIT_SHIFT;
  }
  for (int d = 32; d >= 1; d >>= 1) units += __shfl_xor(units, d, 64);
  const size_t total = units < U ? (size_t)units : U;
  float acc = 0.f;
  for (size_t u = t; u < total; u += 64) acc += part[(size_t)mg * U + u];
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (t == 0) out[mg] = acc;
}

__global__ void masked_copy_kernel(float* __restrict__ dst,
                                   const float* __restrict__ src,
                                   bf16* __restrict__ dlp, size_t n,
                                   const int* __restrict__ mask,
                                   const long long* __restrict__ table, int S,
                                   int vec_ok, size_t n_model) {
  const int mg = blockIdx.y;
  if (mask[mg] == 0) return;
  walk_model_units(
      table, S, mg, (int)gridDim.y, n, n_model, vec_ok,
      [&](size_t e) {
        float4 v = *reinterpret_cast<const float4*>(src + e);
        *reinterpret_cast<float4*>(dst + e) = v;
        if (dlp) store_bf16x4(dlp + e, v);
      },
      [&](size_t e) {
        float v = src[e];
        dst[e] = v;
        if (dlp) dlp[e] = f2bf(v);
      });
}

// walk_model_units between two layouts: the same S tensors, [G_dst,
// per_s] at off_dst[s] in one buffer and [G_src, per_s] at off_src[s]
// in the other. Lane t < S checks segment t against BOTH tables
// (segment_slice on each side; a per that differs between them skips
// the segment too) and the unit table holds the two bases of the pair's
// models gd and gs. vec4(ed, es) / one(ed, es) get the flat element
// index on either side. A segment moves as 16-byte vectors only when
// both of its bases are multiples of 4: off_dst = sum G_dst*per_k can
// be aligned where off_src = sum G_src*per_k is not, and the reverse.
template <class FV, class FS>
MK_DEV_INLINE void walk_pair_units(const long long* __restrict__ dtab,
                                   const long long* __restrict__ stab, int S,
                                   int gd, int G_dst, size_t n_dst,
                                   size_t nm_dst, int gs, int G_src,
                                   size_t n_src, size_t nm_src, int vec_ok,
                                   FV&& vec4, FS&& one) {
  __shared__ size_t sh_dbase[MAX_SEGMENTS], sh_sbase[MAX_SEGMENTS];
  __shared__ size_t sh_per[MAX_SEGMENTS];
  __shared__ size_t sh_units[MAX_SEGMENTS], sh_first[MAX_SEGMENTS];
  __shared__ size_t sh_total;
  __shared__ int sh_seg;
  const int t = threadIdx.x;
  size_t my_units = 0;
  if (t < S) {
    size_t dbase = 0, sbase = 0, dper = 0, sper = 0;
    const bool okd =
        segment_slice(dtab, S, t, gd, G_dst, n_dst, nm_dst, dbase, dper);
    const bool oks =
        segment_slice(stab, S, t, gs, G_src, n_src, nm_src, sbase, sper);
    if (okd && oks && dper == sper)
      my_units = (dper + UNIT - 1) >> UNIT_SHIFT;
    sh_dbase[t] = dbase;
    sh_sbase[t] = sbase;
    sh_per[t] = dper;
    sh_units[t] = my_units;
  }
  __syncthreads();
  size_t my_first = 0;
  if (t < S) {
    for (int j = 0; j < t; ++j) my_first += sh_units[j];
    sh_first[t] = my_first;
    if (t == S - 1) sh_total = my_first + my_units;
  }
  __syncthreads();
  const size_t total = sh_total;
  // the trip count depends on blockIdx and total alone: uniform
  for (size_t u = blockIdx.x; u < total; u += gridDim.x) {
    if (t < S && u >= my_first && u < my_first + my_units) sh_seg = t;
    __syncthreads();
    const int s = sh_seg;
    const size_t dbase = sh_dbase[s], sbase = sh_sbase[s], per = sh_per[s];
    const size_t first = sh_first[s];
    __syncthreads();  // sh_seg is read: the next round may write it
    const size_t lo = (u - first) << UNIT_SHIFT;
    const size_t hi = lo + UNIT < per ? lo + UNIT : per;
    if (vec_ok && (per & 3) == 0 && (dbase & 3) == 0 && (sbase & 3) == 0) {
      const size_t i = lo + ((size_t)threadIdx.x << 2);
      if (i < hi) vec4(dbase + i, sbase + i);  // hi % 4 == 0
    } else {
      for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
        one(dbase + i, sbase + i);
    }
  }
}

// Pack compaction: pair j = blockIdx.y writes the slices of model
// pairs[P + j] of src, in all S tensors, to model pairs[j] of dst (and
// rounded into dst's bf16 mirror). Grid (chunks, P), 256 threads. The
// host entry has validated the pairs; a pair outside either G is
// dropped here as a whole block all the same, before any barrier.
__global__ void remap_models_kernel(
    float* __restrict__ dst, const float* __restrict__ src,
    bf16* __restrict__ dlp, size_t n_dst, size_t n_src,
    const int* __restrict__ pairs, int P, const long long* __restrict__ dtab,
    const long long* __restrict__ stab, int S, int G_dst, int G_src,
    int vec_ok, size_t nm_dst, size_t nm_src) {
  const int gd = pairs[blockIdx.y];
  const int gs = pairs[P + blockIdx.y];
  if (gd < 0 || gd >= G_dst || gs < 0 || gs >= G_src) return;
  walk_pair_units(
      dtab, stab, S, gd, G_dst, n_dst, nm_dst, gs, G_src, n_src, nm_src,
      vec_ok,
      [&](size_t ed, size_t es) {
        float4 v = *reinterpret_cast<const float4*>(src + es);
        *reinterpret_cast<float4*>(dst + ed) = v;
        if (dlp) store_bf16x4(dlp + ed, v);
      },
      [&](size_t ed, size_t es) {
        float v = src[es];
        dst[ed] = v;
        if (dlp) dlp[ed] = f2bf(v);
      });
}

// the step counter bump of the unmasked entries, launched the same way
__global__ void masked_bump_kernel(int* step_buf) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step_buf += 1;
}

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// [2, S] int64 table on p's device; returns S
int check_table(const torch::Tensor& p, const torch::Tensor& table) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt64 &&
                  table.is_contiguous() && table.dim() == 2 &&
                  table.size(0) == 2,
              "the segment table must be a contiguous int64 [2, S] GPU "
              "tensor");
  TORCH_CHECK(table.get_device() == p.get_device(),
              "mask and segment table must live on the buffer's device");
  int64_t S = table.size(1);
  TORCH_CHECK(S >= 1 && S <= MAX_SEGMENTS, "the segment table holds ", S,
              " tensors; the masked kernels take 1 to ", MAX_SEGMENTS);
  return (int)S;
}

// [G] int32 mask and [2, S] int64 table on p's device; returns (G, S)
std::pair<int, int> check_mask_table(const torch::Tensor& p,
                                     const torch::Tensor& mask,
                                     const torch::Tensor& table) {
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kInt32 &&
                  mask.is_contiguous() && mask.dim() == 1,
              "the model mask must be a contiguous int32 [G] GPU tensor");
  TORCH_CHECK(mask.get_device() == p.get_device(),
              "mask and segment table must live on the buffer's device");
  int S = check_table(p, table);
  int64_t G = mask.numel();
  TORCH_CHECK(G >= 1 && G <= 65535, "G must be in [1, 65535]");
  return {(int)G, S};
}

// float32 [2, S] coefficient table beside the segment table
const float* check_reg(const torch::Tensor& p, const torch::Tensor& reg,
                       int S) {
  TORCH_CHECK(reg.is_cuda() && reg.scalar_type() == torch::kFloat32 &&
                  reg.is_contiguous() && reg.dim() == 2 &&
                  reg.size(0) == 2 && reg.size(1) == S &&
                  reg.get_device() == p.get_device(),
              "the regularizer table must be a contiguous float32 [2, S] "
              "tensor on the buffer's device, S that of the segment table");
  return reg.data_ptr<float>();
}

// which optimizer kernel this thread launched last
struct OptLaunch {
  const char* family = "";
  bool reg = false;
};
thread_local OptLaunch g_last_opt;

// blocks per model: one per work unit -- a model has at most
// n/G/1024 + S units (each segment's last unit may be partial) --
// capped so the grid stays near the unmasked entry's 4096 blocks
int chunks_for(size_t n, int G, int S) {
  size_t per_model = n / (size_t)G;
  size_t want = (per_model >> UNIT_SHIFT) + (size_t)S;
  size_t cap = std::max<size_t>(1, 4096 / (size_t)G);
  return (int)std::max<size_t>(1, std::min(want, cap));
}

}  // namespace

namespace gordo_masked {

void note_optimizer_launch(const char* family, bool reg) {
  g_last_opt.family = family;
  g_last_opt.reg = reg;
}

std::tuple<std::string, bool> last_optimizer_launch() {
  return {std::string(g_last_opt.family), g_last_opt.reg};
}

// the masked step (active, no reg), the regularized step (reg, with or
// without active; G then comes from the caller) or both
static void masked_step_impl(int64_t kind, torch::Tensor p, torch::Tensor g,
                             c10::optional<torch::Tensor> s0,
                             c10::optional<torch::Tensor> s1,
                             c10::optional<torch::Tensor> s2,
                             std::vector<double> hyper, bool flag,
                             c10::optional<torch::Tensor> plp,
                             torch::Tensor step_buf,
                             c10::optional<torch::Tensor> active,
                             torch::Tensor table,
                             c10::optional<torch::Tensor> reg, int64_t G_arg) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == torch::kFloat32 &&
                  p.is_contiguous(),
              "p must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == torch::kFloat32 &&
                  g.is_contiguous() && g.numel() == p.numel(),
              "g must match p");
  TORCH_CHECK(step_buf.is_cuda() && step_buf.scalar_type() == torch::kInt32,
              "step_buf must be an int32 GPU tensor");
  TORCH_CHECK(hyper.size() == 4, "hyper must hold 4 values");
  int G, S;
  const int* active_ptr = nullptr;
  if (active.has_value()) {
    auto gs = check_mask_table(p, *active, table);
    G = gs.first, S = gs.second;
    TORCH_CHECK(G_arg <= 0 || G_arg == G, "the mask holds ", G,
                " models, G is ", G_arg);
    active_ptr = active->data_ptr<int>();
  } else {
    TORCH_CHECK(reg.has_value(), "a step without a mask needs reg");
    TORCH_CHECK(G_arg >= 1 && G_arg <= 65535, "G must be in [1, 65535]");
    G = (int)G_arg;
    S = check_table(p, table);
  }
  const float* reg_ptr = reg.has_value() ? check_reg(p, *reg, S) : nullptr;
  size_t n = p.numel();
  bool vec = aligned16(p.data_ptr()) && aligned16(g.data_ptr());
  auto slot = [&](const c10::optional<torch::Tensor>& s, bool needed,
                  const char* name) -> float* {
    if (!needed) return nullptr;
    TORCH_CHECK(s.has_value(), name, " is required for this optimizer");
    TORCH_CHECK(s->is_cuda() && s->scalar_type() == torch::kFloat32 &&
                    s->is_contiguous() && (size_t)s->numel() == n,
                name, " must match p");
    vec = vec && aligned16(s->data_ptr());
    return s->data_ptr<float>();
  };
  bf16* plp_ptr = nullptr;
  if (plp.has_value()) {
    TORCH_CHECK(plp->is_cuda() && plp->scalar_type() == torch::kBFloat16 &&
                    plp->is_contiguous() && (size_t)plp->numel() == n,
                "p_lp must be a bf16 mirror of p");
    plp_ptr = (bf16*)plp->data_ptr();
    vec = vec && aligned16(plp_ptr);
  }
  float h0 = (float)hyper[0], h1 = (float)hyper[1], h2 = (float)hyper[2],
        h3 = (float)hyper[3];
  float *a = nullptr, *b = nullptr, *c = nullptr;
  switch (kind) {
    case OPT_ADAM:
      a = slot(s0, true, "s0");
      b = slot(s1, true, "s1");
      break;
    case OPT_SGD:
      a = slot(s0, h1 != 0.f, "s0");
      break;
    case OPT_RMSPROP:
      a = slot(s0, true, "s0");
      b = slot(s1, h2 > 0.f, "s1");
      break;
    case OPT_ADAGRAD:
      a = slot(s0, true, "s0");
      break;
    case OPT_ADAM_AMSGRAD:
      a = slot(s0, true, "s0");
      b = slot(s1, true, "s1");
      c = slot(s2, true, "s2");
      break;
    case OPT_ADAMAX:
      a = slot(s0, true, "s0");
      b = slot(s1, true, "s1");
      break;
    default:
      TORCH_CHECK(false, "bad optimizer code ", kind);
  }
  hipLaunchKernelGGL(masked_bump_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     step_buf.data_ptr<int>());
  note_optimizer_launch("masked", reg_ptr != nullptr);
  if (n == 0) return;
  TORCH_CHECK(n % (size_t)G == 0, "buffer size must be a multiple of G");
  int chunks = chunks_for(n, G, S);
#define GORDO_MASKED_LAUNCH_R(K, R)                                          \
  hipLaunchKernelGGL((opt_masked_kernel<K, R>), dim3(chunks, G), dim3(256),  \
                     0, cur_stream(), p.data_ptr<float>(),                   \
                     g.data_ptr<float>(), a, b, c, plp_ptr, n, h0, h1, h2,   \
                     h3, flag ? 1 : 0, step_buf.data_ptr<int>(), active_ptr, \
                     (const long long*)table.data_ptr<int64_t>(), S,         \
                     vec ? 1 : 0, n / (size_t)G, reg_ptr)
#define GORDO_MASKED_LAUNCH(K)              \
  do {                                      \
    if (reg_ptr)                            \
      GORDO_MASKED_LAUNCH_R(K, true);       \
    else                                    \
      GORDO_MASKED_LAUNCH_R(K, false);      \
  } while (0)
  switch (kind) {
    case OPT_ADAM: GORDO_MASKED_LAUNCH(OPT_ADAM); break;
    case OPT_SGD: GORDO_MASKED_LAUNCH(OPT_SGD); break;
    case OPT_RMSPROP: GORDO_MASKED_LAUNCH(OPT_RMSPROP); break;
    case OPT_ADAGRAD: GORDO_MASKED_LAUNCH(OPT_ADAGRAD); break;
    case OPT_ADAM_AMSGRAD: GORDO_MASKED_LAUNCH(OPT_ADAM_AMSGRAD); break;
    default: GORDO_MASKED_LAUNCH(OPT_ADAMAX); break;
  }
#undef GORDO_MASKED_LAUNCH
#undef GORDO_MASKED_LAUNCH_R
}

void optimizer_step_masked(int64_t kind, torch::Tensor p, torch::Tensor g,
                           c10::optional<torch::Tensor> s0,
                           c10::optional<torch::Tensor> s1,
                           c10::optional<torch::Tensor> s2,
                           std::vector<double> hyper, bool flag,
                           c10::optional<torch::Tensor> plp,
                           torch::Tensor step_buf, torch::Tensor active,
                           torch::Tensor table) {
  masked_step_impl(kind, p, g, s0, s1, s2, hyper, flag, plp, step_buf, active,
                   table, c10::nullopt, 0);
}

// The segment-aware step with the weight regularizers' gradient term
// fused at the gradient load: `reg` is the float32 [2, S] coefficient
// table (l1 row, l2 row). `active` is optional: without it every one
// of the G models steps.
void optimizer_step_reg(int64_t kind, torch::Tensor p, torch::Tensor g,
                        c10::optional<torch::Tensor> s0,
                        c10::optional<torch::Tensor> s1,
                        c10::optional<torch::Tensor> s2,
                        std::vector<double> hyper, bool flag,
                        c10::optional<torch::Tensor> plp,
                        torch::Tensor step_buf,
                        c10::optional<torch::Tensor> active,
                        torch::Tensor table, torch::Tensor reg, int64_t G) {
  masked_step_impl(kind, p, g, s0, s1, s2, hyper, flag, plp, step_buf, active,
                   table, reg, G);
}

// Per-model penalty sum_s (l1_s sum|w_s| + l2_s sum w_s^2) of the flat
// buffer p, float32 [G]; reads p only (see the two kernels).
torch::Tensor weight_penalty(torch::Tensor p, torch::Tensor table,
                             torch::Tensor reg, int64_t G) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == torch::kFloat32 &&
                  p.is_contiguous(),
              "p must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(G >= 1 && G <= 65535, "G must be in [1, 65535]");
  int S = check_table(p, table);
  const float* reg_ptr = check_reg(p, reg, S);
  size_t n = p.numel();
  auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(p.device());
  if (n == 0) return torch::zeros({G}, opts);
  TORCH_CHECK(n % (size_t)G == 0, "buffer size must be a multiple of G");
  size_t n_model = n / (size_t)G;
  // a model has at most n/G/1024 + S units (chunks_for); a table whose
  // segments overlap could name more, and those are dropped
  size_t U = (n_model >> UNIT_SHIFT) + (size_t)S;
  auto part = torch::empty({G, (int64_t)U}, opts);
  auto out = torch::empty({G}, opts);
  int chunks = chunks_for(n, (int)G, S);
  const long long* tab = (const long long*)table.data_ptr<int64_t>();
  hipLaunchKernelGGL(weight_penalty_units_kernel, dim3(chunks, (unsigned)G),
                     dim3(256), 0, cur_stream(), p.data_ptr<float>(), n, tab,
                     reg_ptr, S, aligned16(p.data_ptr()) ? 1 : 0, n_model,
                     part.data_ptr<float>(), U);
  hipLaunchKernelGGL(weight_penalty_sum_kernel, dim3((unsigned)G), dim3(64),
                     0, cur_stream(), part.data_ptr<float>(), U, tab, S,
                     (int)G, n, n_model, out.data_ptr<float>());
  return out;
}

void masked_copy(torch::Tensor dst, torch::Tensor src, torch::Tensor mask,
                 torch::Tensor table, c10::optional<torch::Tensor> dst_lp) {
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == torch::kFloat32 &&
                  dst.is_contiguous(),
              "dst must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == torch::kFloat32 &&
                  src.is_contiguous() && src.numel() == dst.numel() &&
                  src.get_device() == dst.get_device(),
              "src must match dst");
  auto gs = check_mask_table(dst, mask, table);
  int G = gs.first, S = gs.second;
  size_t n = dst.numel();
  bool vec = aligned16(dst.data_ptr()) && aligned16(src.data_ptr());
  bf16* lp_ptr = nullptr;
  if (dst_lp.has_value()) {
    TORCH_CHECK(dst_lp->is_cuda() &&
                    dst_lp->scalar_type() == torch::kBFloat16 &&
                    dst_lp->is_contiguous() && (size_t)dst_lp->numel() == n,
                "dst_lp must be a bf16 mirror of dst");
    lp_ptr = (bf16*)dst_lp->data_ptr();
    vec = vec && aligned16(lp_ptr);
  }
  if (n == 0) return;
  TORCH_CHECK(n % (size_t)G == 0, "buffer size must be a multiple of G");
  int chunks = chunks_for(n, G, S);
  hipLaunchKernelGGL(masked_copy_kernel, dim3(chunks, G), dim3(256), 0,
                     cur_stream(), dst.data_ptr<float>(),
                     src.data_ptr<float>(), lp_ptr, n, mask.data_ptr<int>(),
                     (const long long*)table.data_ptr<int64_t>(), S,
                     vec ? 1 : 0, n / (size_t)G);
}

void remap_models(torch::Tensor dst, torch::Tensor src,
                  std::vector<int64_t> dst_index,
                  std::vector<int64_t> src_index, torch::Tensor dst_table,
                  torch::Tensor src_table, int64_t G_dst, int64_t G_src,
                  c10::optional<torch::Tensor> dst_lp) {
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == torch::kFloat32 &&
                  dst.is_contiguous(),
              "dst must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == torch::kFloat32 &&
                  src.is_contiguous() &&
                  src.get_device() == dst.get_device(),
              "src must be a contiguous fp32 tensor on dst's device");
  TORCH_CHECK(G_dst >= 1 && G_dst <= 65535 && G_src >= 1 && G_src <= 65535,
              "G_dst and G_src must be in [1, 65535]");
  for (const torch::Tensor* t : {&dst_table, &src_table}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kInt64 &&
                    t->is_contiguous() && t->dim() == 2 && t->size(0) == 2 &&
                    t->get_device() == dst.get_device(),
                "a segment table must be a contiguous int64 [2, S] tensor "
                "on the buffers' device");
  }
  int64_t S = dst_table.size(1);
  TORCH_CHECK(src_table.size(1) == S,
              "the two segment tables must hold the same tensors");
  TORCH_CHECK(S >= 1 && S <= MAX_SEGMENTS, "the segment table holds ", S,
              " tensors; the masked kernels take 1 to ", MAX_SEGMENTS);
  // the pairs, checked on the host: nothing below may launch on a
  // list that leaves either buffer
  size_t P = dst_index.size();
  TORCH_CHECK(P >= 1 && src_index.size() == P,
              "dst_index and src_index must have the same length >= 1");
  std::vector<char> seen((size_t)G_dst, 0);
  for (size_t j = 0; j < P; ++j) {
    TORCH_CHECK(dst_index[j] >= 0 && dst_index[j] < G_dst,
                "dst_index[", j, "] = ", dst_index[j], " is outside [0, ",
                G_dst, ")");
    TORCH_CHECK(src_index[j] >= 0 && src_index[j] < G_src,
                "src_index[", j, "] = ", src_index[j], " is outside [0, ",
                G_src, ")");
    TORCH_CHECK(!seen[(size_t)dst_index[j]], "dst_index holds model ",
                dst_index[j], " twice");
    seen[(size_t)dst_index[j]] = 1;
  }
  size_t n_dst = dst.numel(), n_src = src.numel();
  TORCH_CHECK(n_dst % (size_t)G_dst == 0 && n_src % (size_t)G_src == 0,
              "each buffer's size must be a multiple of its G");
  bool vec = aligned16(dst.data_ptr()) && aligned16(src.data_ptr());
  bf16* lp_ptr = nullptr;
  if (dst_lp.has_value()) {
    TORCH_CHECK(dst_lp->is_cuda() &&
                    dst_lp->scalar_type() == torch::kBFloat16 &&
                    dst_lp->is_contiguous() &&
                    (size_t)dst_lp->numel() == n_dst &&
                    dst_lp->get_device() == dst.get_device(),
                "dst_lp must be a bf16 mirror of dst");
    lp_ptr = (bf16*)dst_lp->data_ptr();
    vec = vec && aligned16(lp_ptr);
  }
  if (n_dst == 0 || n_src == 0) return;
  // both index lists travel as one int32 [2, P] tensor
  auto pairs_h = torch::empty({2, (int64_t)P}, torch::kInt32);
  int* ph = pairs_h.data_ptr<int>();
  for (size_t j = 0; j < P; ++j) {
    ph[j] = (int)dst_index[j];
    ph[P + j] = (int)src_index[j];
  }
  auto pairs = pairs_h.to(dst.device());
  // one block per unit of a model, as chunks_for, with the grid capped
  // by the number of pairs
  size_t want = ((n_dst / (size_t)G_dst) >> UNIT_SHIFT) + (size_t)S;
  size_t cap = std::max<size_t>(1, 4096 / P);
  int chunks = (int)std::max<size_t>(1, std::min(want, cap));
  hipLaunchKernelGGL(remap_models_kernel, dim3(chunks, (unsigned)P),
                     dim3(256), 0, cur_stream(), dst.data_ptr<float>(),
                     src.data_ptr<float>(), lp_ptr, n_dst, n_src,
                     pairs.data_ptr<int>(), (int)P,
                     (const long long*)dst_table.data_ptr<int64_t>(),
                     (const long long*)src_table.data_ptr<int64_t>(), (int)S,
                     (int)G_dst, (int)G_src, vec ? 1 : 0,
                     n_dst / (size_t)G_dst, n_src / (size_t)G_src);
}

}  // namespace gordo_masked
