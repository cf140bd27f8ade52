// Device smoothing kernels for MI355X (gfx950) — SURVEY.md §2.3 K11:
// the three `smoothing_method`s of the DiffBased detectors (smm, sma,
// ewma) as one op,
//
//   smooth(X [R, N] fp32, w, method) -> fp64 [R, N]
//
// series-major like K10-K12 (callers transpose with torch) and with the
// full pandas-shaped output, so the serving frames assemble without
// padding. fp64 out on purpose: pandas returns float64 from float32
// input, and the frames keep that dtype and precision.
//
// Semantics (pinned against reference.smooth_ref, an fp64 oracle, by
// tests/test_smoothing_gpu.py; the oracle against pandas by
// tests/test_smoothing_oracle.py):
//  * Missing values: NaN, +inf and -inf are MISSING in all three
//    methods, as in pandas rolling().mean()/median() and ewm().mean().
//    (K10-K12 of thresholds.hip keep their own documented +-inf rule.)
//  * smm (method 0) = rolling(w).median(), min_periods = w: positions
//    < w-1 are NaN, a window holding any missing value is NaN, odd w
//    gives the middle order statistic, even w gives (a + b) / 2 formed
//    in double — exact for fp32 inputs, so smm equals the oracle bit
//    for bit.
//  * sma (method 1) = rolling(w).mean(), min_periods = w, same NaN
//    rule. The window sum is formed in fp64 from THAT window's own
//    values, in ascending time order: no prefix-sum difference and no
//    add/remove running sum, so a 1e30 three windows back does not
//    touch a window of 1e-3 values (an uncompensated running sum is off
//    there by 1e30 * 2^-53).
//  * ewma (method 2) = ewm(span=w, adjust=True, ignore_na=False,
//    min_periods=0).mean(), alpha = 2/(w+1): num and den both decay by
//    (1-alpha) at every position, a valid value adds x to num and 1 to
//    den; the output is num/den at a valid position, a missing
//    position repeats the last output, and it is NaN before the first
//    valid value. All in fp64.
//  * Limits: w >= 1 (else raises); smm w <= 8192 (else raises); w > N
//    gives an all-NaN output for smm and sma (as pandas does);
//    R*N <= INT32_MAX; R == 0 or N == 0 returns empty.
//  * Deterministic: no atomics, fixed summation orders; results are
//    bitwise identical across launches.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <tuple>

#define DEV_INLINE __device__ __forceinline__

namespace {

// missing = NaN or +-inf (one compare: |x| < inf is false for all three)
DEV_INLINE bool is_missing(float v) { return !(fabsf(v) < INFINITY); }

DEV_INLINE float bcast_lane(float v, int lane) {
  return __int_as_float(
      __builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---------------------------------------------------------------------------
// smm: sliding sorted window. One 64-lane workgroup (one wave) per
// (row, chunk of SMM_CHUNK outputs). The wave loads the chunk's first
// window into LDS with missing values replaced by a +inf sentinel,
// bitonic-sorts it once, then slides: per step it finds the rank of the
// outgoing and of the incoming value (each lane compares its
// ceil(w/64) elements, 64-bit __ballot + popcount), and copies the
// window into the second LDS buffer with the elements between the two
// ranks shifted by one. A sliding integer count of missing values
// decides NaN. Results stay in lane registers (lane s keeps step s)
// and leave in one coalesced store.
// LDS: 2 * next_pow2(w) floats per wave = 64 KiB at w = 8192, which is
// why the workgroup is a single wave.
// ---------------------------------------------------------------------------
constexpr int SMM_CHUNK = 64;   // outputs per wave
constexpr int SMM_MAX_W = 8192;

__global__ __launch_bounds__(64) void smm_slide_kernel(
    const float* __restrict__ X, double* __restrict__ out, int N, int w,
    int P, int chunks) {
  extern __shared__ float smm_lds[];  // two buffers of P floats
  float* A = smm_lds;
  float* B = smm_lds + P;
  const int lane = threadIdx.x;
  const int r = blockIdx.x / chunks;
  const int c = blockIdx.x % chunks;
  const float* row = X + (size_t)r * N;
  double* orow = out + (size_t)r * N;
  const int c0 = w - 1 + c * SMM_CHUNK;          // first output position
  const int nsteps = min(SMM_CHUNK, N - c0);     // >= 1 by the grid

  if (c == 0)  // min_periods = w: the head of the row
    for (int i = lane; i < w - 1; i += 64) orow[i] = NAN;

  // first window [c0-w+1, c0] -> A, sentinel for missing and for pad
  int nmiss = 0;
  for (int base = 0; base < P; base += 64) {
    const int k = base + lane;
    float v = INFINITY;
    bool miss = false;
    if (k < w) {
      v = row[c0 - w + 1 + k];
      miss = is_missing(v);
      if (miss) v = INFINITY;
    }
    if (k < P) A[k] = v;  // P < 64 for short windows
    nmiss += __popcll(__ballot(miss));
  }
  // the chunk's incoming and outgoing values, one per lane: step s > 0
  // inserts row[c0+s] and removes row[c0+s-w]
  float in_v = INFINITY, out_v = INFINITY;
  if (lane >= 1 && lane < nsteps) {
    in_v = row[c0 + lane];
    out_v = row[c0 + lane - w];
  }
  __syncthreads();
  // bitonic sort of A[0, P), ascending (pads are +inf and stay on top)
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = lane; idx < P; idx += 64) {
        const int ixj = idx ^ j;
        if (ixj > idx) {
          const float a = A[idx], b = A[ixj];
          const bool up = ((idx & k) == 0);
          if ((a > b) == up) { A[idx] = b; A[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }

  const int mid_lo = (w - 1) >> 1, mid_hi = w >> 1;
  double res = NAN;
  for (int s = 0; s < nsteps; ++s) {
    if (s > 0) {
      float o = bcast_lane(out_v, s);
      float v = bcast_lane(in_v, s);
      const bool om = is_missing(o), vm = is_missing(v);
      if (om) o = INFINITY;
      if (vm) v = INFINITY;
      nmiss += (vm ? 1 : 0) - (om ? 1 : 0);
      // ranks: ro = index of the first element equal to o; rv = where
      // v goes once that element is gone
      int ro = 0, rv = 0;
      for (int base = 0; base < w; base += 64) {
        const int k = base + lane;
        const float x = k < w ? A[k] : INFINITY;  // inf < anything: never
        ro += __popcll(__ballot(x < o));
        rv += __popcll(__ballot(x < v));
      }
      rv -= (o < v) ? 1 : 0;
      for (int base = 0; base < w; base += 64) {
        const int k = base + lane;
        if (k < w && k != ro) {
          int kp = k - (k > ro ? 1 : 0);
          kp += (kp >= rv ? 1 : 0);
          B[kp] = A[k];
        }
      }
      if (lane == 0) B[rv] = v;
      float* t = A; A = B; B = t;
      __syncthreads();
    }
    const float a = A[mid_lo], b = A[mid_hi];
    if (lane == s)
      res = nmiss > 0 ? (double)NAN : ((double)a + (double)b) * 0.5;
  }
  if (lane < nsteps) orow[c0 + lane] = res;
}

// ---------------------------------------------------------------------------
// sma: lanes along time. One 256-thread workgroup per (row, SMA_TILE
// outputs). The window is walked in segments of SMA_SEG positions; per
// segment the workgroup stages segment + tile halo in LDS as
// (value-or-0, missing flag) pairs, then every thread adds its own
// window's part of the segment in ascending time order in fp64 and
// counts the flags. Any w fits: the LDS size does not depend on it.
// ---------------------------------------------------------------------------
constexpr int SMA_TILE = 256;   // outputs per workgroup = threads
constexpr int SMA_SEG = 1024;   // window positions staged per pass

__global__ __launch_bounds__(256) void sma_window_kernel(
    const float* __restrict__ X, double* __restrict__ out, int N, int w,
    int tiles) {
  __shared__ float2 st[SMA_SEG + SMA_TILE];  // .x value-or-0, .y flag bits
  const int tid = threadIdx.x;
  const int r = blockIdx.x / tiles;
  const int c = blockIdx.x % tiles;
  const float* row = X + (size_t)r * N;
  double* orow = out + (size_t)r * N;
  const int c0 = w - 1 + c * SMA_TILE;  // first output position
  // compared as differences: N may be within 256 of INT32_MAX
  const bool active = tid < N - c0;     // this thread's output is c0 + tid

  if (c == 0)
    for (int k = tid; k < w - 1; k += 256) orow[k] = NAN;

  double acc = 0.0;
  int miss = 0;
  for (int k0 = 0; k0 < w; k0 += SMA_SEG) {
    const int seglen = min(SMA_SEG, w - k0);
    const int base = c0 - (w - 1) + k0;  // >= 0
    const int count = seglen + SMA_TILE - 1;
    __syncthreads();  // the previous segment has been read
    // slots past the row's end are read by inactive threads only
    const int left = N - base;
    for (int j = tid; j < count; j += 256) {
      float v = j < left ? row[base + j] : 0.f;
      const bool bad = is_missing(v);
      st[j] = make_float2(bad ? 0.f : v, __int_as_float(bad ? 1 : 0));
    }
    __syncthreads();
    if (active) {
      for (int k = 0; k < seglen; ++k) {
        const float2 e = st[tid + k];
        acc += (double)e.x;
        miss += __float_as_int(e.y);
      }
    }
  }
  if (active) orow[c0 + tid] = miss > 0 ? (double)NAN : acc / (double)w;
}

// ---------------------------------------------------------------------------
// ewma: one wave per row walks the row in blocks of 64 positions. In a
// block, a 6-step shuffle scan with factors d^(2^m), d = 1 - alpha,
// gives every lane num and den over the block; the carry of the
// previous block enters as d^(lane+1) * carry. The powers d^(2^m),
// m = 0..6, are formed once per launch on the host. A missing position
// takes the output of the last valid one (max-scan of the valid lane
// index), across blocks through `last`.
// ---------------------------------------------------------------------------
struct EwmaPowers {
  double f[7];  // d^(2^m)
};

__global__ __launch_bounds__(64) void ewma_scan_kernel(
    const float* __restrict__ X, double* __restrict__ out, int N,
    EwmaPowers pw) {
  const int lane = threadIdx.x;
  const int r = blockIdx.x;
  const float* row = X + (size_t)r * N;
  double* orow = out + (size_t)r * N;

  double lanepow = 1.0;  // d^(lane+1)
#pragma unroll
  for (int m = 0; m < 7; ++m)
    if (((lane + 1) >> m) & 1) lanepow *= pw.f[m];

  double cnum = 0.0, cden = 0.0;  // carry: num, den at the block's end
  double last = NAN;              // output of the last valid position
  float nxt = lane < N ? row[lane] : NAN;
  const int nblocks = (N - 1) / 64 + 1;  // N >= 1; no sum past INT32_MAX
  for (int b = 0; b < nblocks; ++b) {
    const int b0 = b * 64;
    const int left = N - b0;  // positions from b0 to the row's end
    const float xv = nxt;
    nxt = 64 + lane < left ? row[b0 + 64 + lane] : NAN;  // next block
    const bool valid = !is_missing(xv);  // lanes past N are missing
    double num = valid ? (double)xv : 0.0;
    double den = valid ? 1.0 : 0.0;
    int vi = valid ? lane : -1;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      const int d = 1 << m;
      const double yn = __shfl_up(num, d, 64);
      const double yd = __shfl_up(den, d, 64);
      const int yi = __shfl_up(vi, d, 64);
      if (lane >= d) {
        num += pw.f[m] * yn;
        den += pw.f[m] * yd;
        vi = max(vi, yi);
      }
    }
    num += lanepow * cnum;
    den += lanepow * cden;
    // den >= 1 at a valid lane
    const double own = valid ? num / den : 0.0;
    const double got = __shfl(own, vi < 0 ? 0 : vi, 64);
    const double o = vi < 0 ? last : got;
    if (lane < left) orow[b0 + lane] = o;
    cnum = __shfl(num, 63, 64);
    cden = __shfl(den, 63, 64);
    last = __shfl(o, 63, 64);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
namespace gordo_smoothing {

static inline void check_launch(const char* kernel) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, kernel, " launch failed: ",
              hipGetErrorString(err));
}

static inline int next_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

struct SmoothLaunch {
  const char* method = "";
  const char* family = "";
  int64_t rows = 0, n = 0, window = 0;
};
thread_local SmoothLaunch g_last_smooth;

std::tuple<std::string, std::string, int64_t, int64_t, int64_t>
last_smooth_launch() {
  return {std::string(g_last_smooth.method),
          std::string(g_last_smooth.family), g_last_smooth.rows,
          g_last_smooth.n, g_last_smooth.window};
}

torch::Tensor smooth(torch::Tensor X, int64_t w, int64_t method) {
  TORCH_CHECK(X.is_cuda() && X.dim() == 2, "X must be [R, N] on GPU");
  TORCH_CHECK(method >= 0 && method <= 2,
              "method must be 0 (smm), 1 (sma) or 2 (ewma)");
  TORCH_CHECK(w >= 1, "window must be at least 1");
  TORCH_CHECK(method != 0 || w <= SMM_MAX_W,
              "window too large for the smm LDS window (max 8192)");
  static const char* const names[3] = {"smm", "sma", "ewma"};
  auto xc = X.to(torch::kFloat32).contiguous();
  const int64_t R = xc.size(0), N = xc.size(1);
  TORCH_CHECK(R * N <= INT32_MAX, "too many elements for one launch");
  auto opts = xc.options().dtype(torch::kFloat64);
  auto record = [&](const char* family) {
    g_last_smooth = SmoothLaunch{names[method], family, R, N, w};
  };
  if (R == 0 || N == 0) {
    record("empty");
    return torch::empty({R, N}, opts);
  }
  if (method != 2 && w > N) {  // no full window: all NaN, as pandas
    record("nan_fill");
    return torch::full({R, N}, std::numeric_limits<double>::quiet_NaN(),
                       opts);
  }
  auto out = torch::empty({R, N}, opts);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const float* xp = xc.data_ptr<float>();
  double* op = out.data_ptr<double>();
  const int n = (int)N, wi = (int)w;
  if (method == 0) {
    const int no = n - wi + 1;
    const int chunks = (no + SMM_CHUNK - 1) / SMM_CHUNK;
    const int P = std::max(next_pow2(wi), 2);
    hipLaunchKernelGGL(smm_slide_kernel, dim3((unsigned)(R * chunks)),
                       dim3(64), 2 * (size_t)P * sizeof(float), stream, xp,
                       op, n, wi, P, chunks);
    check_launch("smm_slide_kernel");
    record("smm_slide");
  } else if (method == 1) {
    const int no = n - wi + 1;
    const int tiles = (no + SMA_TILE - 1) / SMA_TILE;
    hipLaunchKernelGGL(sma_window_kernel, dim3((unsigned)(R * tiles)),
                       dim3(256), 0, stream, xp, op, n, wi, tiles);
    check_launch("sma_window_kernel");
    record("sma_window");
  } else {
    EwmaPowers pw;
    const double alpha = 2.0 / ((double)w + 1.0);
    pw.f[0] = 1.0 - alpha;
    for (int m = 1; m < 7; ++m) pw.f[m] = pw.f[m - 1] * pw.f[m - 1];
    hipLaunchKernelGGL(ewma_scan_kernel, dim3((unsigned)R), dim3(64), 0,
                       stream, xp, op, n, pw);
    check_launch("ewma_scan_kernel");
    record("ewma_scan");
  }
  return out;
}

}  // namespace gordo_smoothing
