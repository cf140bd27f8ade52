// Train-step ops that honour the compile settings of a pack:
//   loss_bwd        one pass over (Y, T): per-model loss (mse / mae /
//                   huber / logcosh), its gradient, and the Keras
//                   "accuracy" count (categorical argmax match, or
//                   binary accuracy for a single output column).
//   optimizer_step  fused SGD / RMSprop / Adagrad / Adam(amsgrad) /
//                   Adamax over the flat fp32 master buffer + bf16
//                   mirror refresh. Plain Adam keeps its own kernel in
//                   gordo_kernels.hip.
//
// loss_bwd is organised by ROWS (the argmax is a per-row reduction):
// L lanes cooperate on one row, L = smallest power of two >=
// ceil(Fp/8) capped at 64, so a wave covers 64/L rows and each lane
// moves 16-byte bf16x8 vectors when Fp % 8 == 0 (the pad8 layout).
// Rows wider than 64 lanes x 8 elements loop.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

#define TO_DEV_INLINE __device__ __forceinline__

using bf16 = __hip_bfloat16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// loss codes (keep in sync with gordo_amd/ops/reference.py)
constexpr int LOSS_MSE = 0, LOSS_MAE = 1, LOSS_HUBER = 2, LOSS_LOGCOSH = 3;
// optimizer codes (plain Adam = 0 never reaches this file)
constexpr int OPT_SGD = 1, OPT_RMSPROP = 2, OPT_ADAGRAD = 3,
              OPT_ADAM_AMSGRAD = 4, OPT_ADAMAX = 5;

TO_DEV_INLINE float bf2f(bf16 v) { return __bfloat162float(v); }
TO_DEV_INLINE bf16 f2bf(float v) { return __float2bfloat16(v); }

TO_DEV_INLINE float fast_tanhf(float x) {
  float e = __expf(2.f * x);
  return 1.f - 2.f / (e + 1.f);  // saturates to 1 when e overflows to inf
}

TO_DEV_INLINE float sign0(float d) {
  return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
}

// per-element loss l(d) and dl/dd; every loss has l(0) = 0 and a zero
// gradient at 0, so zero-padded feature columns stay inert.
TO_DEV_INLINE void loss_elem(int kind, float d, float delta, float& l,
                             float& gr) {
  float a = fabsf(d);
  switch (kind) {
    case LOSS_MAE:
      l = a;
      gr = sign0(d);
      break;
    case LOSS_HUBER:
      if (a <= delta) {
        l = 0.5f * d * d;
        gr = d;
      } else {
        l = delta * (a - 0.5f * delta);
        gr = delta * sign0(d);
      }
      break;
    case LOSS_LOGCOSH:
      // log(cosh d) = |d| + log1p(exp(-2|d|)) - log 2 (no overflow).
      // d == 0 is pinned to exactly 0: log1pf(1) need not round to the
      // same float as the constant, and pad columns must add nothing.
      l = a == 0.f ? 0.f : a + log1pf(__expf(-2.f * a)) - 0.69314718056f;
      gr = fast_tanhf(d);
      break;
    default:  // LOSS_MSE — same expression as mse_bwd_kernel
      l = d * d;
      gr = 2.f * d;
      break;
  }
}

// running (max, first index) — strict ordering with ties to the lowest
// column, the rule torch.argmax / np.argmax document. A NaN ranks above
// every number (the first NaN wins), as torch.argmax has it, so the
// count of a diverged model still agrees with the CPU reference.
struct ArgMax {
  float v;
  int i;
};

TO_DEV_INLINE void argmax_take(ArgMax& a, float v, int i) {
  const bool vn = v != v, an = a.v != a.v;
  const bool better = vn ? !an : (!an && v > a.v);
  const bool same = vn ? an : v == a.v;
  if (better || (same && i < a.i)) {
    a.v = v;
    a.i = i;
  }
}

template <bool VEC>
__global__ void loss_bwd_kernel(const bf16* __restrict__ Y,
                                const bf16* __restrict__ T,
                                bf16* __restrict__ dY,  // null: no grad
                                float* __restrict__ loss,
                                int* __restrict__ correct, int B, int Fp,
                                int real_f, int L, int kind, float delta) {
  const int g = blockIdx.y;
  const size_t per_g = (size_t)B * Fp;
  const bf16* Yg = Y + (size_t)g * per_g;
  const bf16* Tg = T + (size_t)g * per_g;
  bf16* dYg = dY ? dY + (size_t)g * per_g : nullptr;
  const float inv_n = 1.f / (float)(B * real_f);

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  const int rows_per_wave = 64 / L;
  const int rows_per_block = rows_per_wave * waves;
  const int sub = lane & (L - 1);  // lane within the row
  const int row_in_wave = lane / L;

  float local = 0.f;
  int hits = 0;
  // the trip count is uniform per block, so every lane reaches the
  // shuffles below; rows past B only skip their memory traffic
  for (int base = blockIdx.x * rows_per_block; base < B;
       base += gridDim.x * rows_per_block) {
    const int row = base + wid * rows_per_wave + row_in_wave;
    const bool live = row < B;
    ArgMax ay{-INFINITY, INT_MAX}, at{-INFINITY, INT_MAX};
    if (live) {
      const size_t roff = (size_t)row * Fp;
      for (int c0 = sub * 8; c0 < Fp; c0 += L * 8) {
        alignas(16) bf16 yv[8], tv[8], gv[8];
        if (VEC) {
          *reinterpret_cast<u32x4*>(yv) =
              *reinterpret_cast<const u32x4*>(Yg + roff + c0);
          *reinterpret_cast<u32x4*>(tv) =
              *reinterpret_cast<const u32x4*>(Tg + roff + c0);
        } else {
          #pragma unroll
          for (int e = 0; e < 8; ++e) {
            bool in = c0 + e < Fp;
            yv[e] = in ? Yg[roff + c0 + e] : f2bf(0.f);
            tv[e] = in ? Tg[roff + c0 + e] : f2bf(0.f);
          }
        }
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
          float y = bf2f(yv[e]), t = bf2f(tv[e]);
          float l, gr;
          loss_elem(kind, y - t, delta, l, gr);
          local += l;
          gv[e] = f2bf(gr * inv_n);
          // pad columns (>= real_f) never enter the argmax: a padded 0
          // would beat an all-negative row
          if (c0 + e < real_f) {
            argmax_take(ay, y, c0 + e);
            argmax_take(at, t, c0 + e);
          }
        }
        if (dYg) {
          if (VEC) {
            *reinterpret_cast<u32x4*>(dYg + roff + c0) =
                *reinterpret_cast<const u32x4*>(gv);
          } else {
            #pragma unroll
            for (int e = 0; e < 8; ++e)
              if (c0 + e < Fp) dYg[roff + c0 + e] = gv[e];
          }
        }
      }
    }
    // segmented butterfly over the L lanes of the row
    for (int off = L >> 1; off; off >>= 1) {
      float ov = __shfl_xor(ay.v, off, 64);
      int oi = __shfl_xor(ay.i, off, 64);
      argmax_take(ay, ov, oi);
      ov = __shfl_xor(at.v, off, 64);
      oi = __shfl_xor(at.i, off, 64);
      argmax_take(at, ov, oi);
    }
    if (live && sub == 0) {
      bool ok = real_f == 1
                    ? (at.v == (ay.v > 0.5f ? 1.f : 0.f))  // binary accuracy
                    : (ay.i == at.i);
      hits += ok ? 1 : 0;
    }
  }
  // wave -> block -> global reduction
  #pragma unroll
  for (int off = 32; off; off >>= 1) {
    local += __shfl_down(local, off, 64);
    hits += __shfl_down(hits, off, 64);
  }
  __shared__ float loss_part[4];
  __shared__ int hit_part[4];
  if (lane == 0) {
    loss_part[wid] = local;
    hit_part[wid] = hits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    int h = 0;
    for (int w = 0; w < waves; ++w) {
      s += loss_part[w];
      h += hit_part[w];
    }
    atomicAdd(&loss[g], s * inv_n);
    if (h) atomicAdd(&correct[g], h);
  }
}

// device-resident step counter, bumped on the stream so a captured
// sequence recomputes its bias correction at every replay
__global__ void opt_bump_kernel(int* step_buf) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step_buf += 1;
}

// h0..h3 per kind:
//   SGD           lr, momentum               flag = nesterov
//   RMSprop       lr, rho, momentum, eps
//   Adagrad       lr, eps
//   Adam+amsgrad  lr, beta1, beta2, eps
//   Adamax        lr, beta1, beta2, eps
template <int KIND>
__global__ void opt_kernel(float* __restrict__ p, const float* __restrict__ g,
                           float* __restrict__ s0, float* __restrict__ s1,
                           float* __restrict__ s2, bf16* __restrict__ plp,
                           size_t n, float h0, float h1, float h2, float h3,
                           int flag, const int* __restrict__ step_buf) {
  float bc1 = 1.f, bc2 = 1.f;
  if (KIND == OPT_ADAM_AMSGRAD || KIND == OPT_ADAMAX) {
    float fstep = (float)*step_buf;
    bc1 = 1.f - powf(h1, fstep);
    bc2 = 1.f - powf(h2, fstep);
  }
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float gi = g[i];
    float pi = p[i];
    if (KIND == OPT_SGD) {
      if (h1 == 0.f) {
        pi -= h0 * gi;
      } else {
        float mi = h1 * s0[i] - h0 * gi;
        s0[i] = mi;
        pi += flag ? h1 * mi - h0 * gi : mi;
      }
    } else if (KIND == OPT_RMSPROP) {
      float vi = h1 * s0[i] + (1.f - h1) * gi * gi;
      s0[i] = vi;
      float inc = h0 * gi / sqrtf(vi + h3);
      if (h2 > 0.f) {
        float mi = h2 * s1[i] + inc;
        s1[i] = mi;
        pi -= mi;
      } else {
        pi -= inc;
      }
    } else if (KIND == OPT_ADAGRAD) {
      float ai = s0[i] + gi * gi;
      s0[i] = ai;
      pi -= h0 * gi / sqrtf(ai + h1);
    } else if (KIND == OPT_ADAM_AMSGRAD) {
      float mi = h1 * s0[i] + (1.f - h1) * gi;
      float vi = h2 * s1[i] + (1.f - h2) * gi * gi;
      float vh = fmaxf(s2[i], vi);
      s0[i] = mi;
      s1[i] = vi;
      s2[i] = vh;
      pi -= h0 * sqrtf(bc2) / bc1 * mi / (sqrtf(vh) + h3);
    } else {  // OPT_ADAMAX
      float mi = h1 * s0[i] + (1.f - h1) * gi;
      float ui = fmaxf(h2 * s1[i], fabsf(gi));
      s0[i] = mi;
      s1[i] = ui;
      pi -= h0 / bc1 * mi / (ui + h3);
    }
    p[i] = pi;
    if (plp) plp[i] = f2bf(pi);
  }
}

hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// the optimizer launch record lives in masked_ops.hip
namespace gordo_masked {
void note_optimizer_launch(const char* family, bool reg);
}

namespace gordo_train {

std::vector<torch::Tensor> loss_bwd(torch::Tensor Y, torch::Tensor T,
                                    int64_t kind, int64_t real_f,
                                    double delta, bool want_grad) {
  TORCH_CHECK(Y.is_cuda() && Y.dim() == 3, "Y must be [G,B,Fp] on GPU");
  TORCH_CHECK(T.sizes() == Y.sizes(), "Y/T shape mismatch");
  TORCH_CHECK(kind >= LOSS_MSE && kind <= LOSS_LOGCOSH, "bad loss code");
  auto Yc = Y.to(torch::kBFloat16).contiguous();
  auto Tc = T.to(torch::kBFloat16).contiguous();
  int64_t G = Yc.size(0), B = Yc.size(1), Fp = Yc.size(2);
  TORCH_CHECK(real_f >= 1 && real_f <= Fp, "real_f must be in [1, Fp]");
  TORCH_CHECK(B * Fp < ((int64_t)1 << 31), "per-model batch too large");
  auto loss = torch::zeros({G}, Yc.options().dtype(torch::kFloat32));
  auto correct = torch::zeros({G}, Yc.options().dtype(torch::kInt32));
  torch::Tensor dY;
  bf16* dY_ptr = nullptr;
  if (want_grad) {
    dY = torch::empty_like(Yc);
    dY_ptr = (bf16*)dY.data_ptr();
  }
  if (G == 0 || B == 0) return {loss, dY, correct};
  int chunks = (int)((Fp + 7) / 8);
  int L = 1;
  while (L < chunks && L < 64) L <<= 1;
  int rows_per_block = (64 / L) * 4;
  int blocks =
      (int)std::min<int64_t>((B + rows_per_block - 1) / rows_per_block, 512);
  bool vec = Fp % 8 == 0 && aligned16(Yc.data_ptr()) &&
             aligned16(Tc.data_ptr()) && (!dY_ptr || aligned16(dY_ptr));
  auto launch = vec ? loss_bwd_kernel<true> : loss_bwd_kernel<false>;
  hipLaunchKernelGGL(launch, dim3(blocks, (unsigned)G), dim3(256), 0,
                     cur_stream(), (const bf16*)Yc.data_ptr(),
                     (const bf16*)Tc.data_ptr(), dY_ptr,
                     loss.data_ptr<float>(), correct.data_ptr<int>(), (int)B,
                     (int)Fp, (int)real_f, L, (int)kind, (float)delta);
  return {loss, dY, correct};
}

void optimizer_step(int64_t kind, torch::Tensor p, torch::Tensor g,
                    c10::optional<torch::Tensor> s0,
                    c10::optional<torch::Tensor> s1,
                    c10::optional<torch::Tensor> s2,
                    std::vector<double> hyper, bool flag,
                    c10::optional<torch::Tensor> plp,
                    torch::Tensor step_buf) {
  TORCH_CHECK(p.is_cuda() && p.scalar_type() == torch::kFloat32 &&
                  p.is_contiguous(),
              "p must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == torch::kFloat32 &&
                  g.is_contiguous() && g.numel() == p.numel(),
              "g must match p");
  TORCH_CHECK(step_buf.is_cuda() && step_buf.scalar_type() == torch::kInt32,
              "step_buf must be an int32 GPU tensor");
  TORCH_CHECK(hyper.size() == 4, "hyper must hold 4 values");
  size_t n = p.numel();
  auto slot = [&](const c10::optional<torch::Tensor>& s, bool needed,
                  const char* name) -> float* {
    if (!needed) return nullptr;
    TORCH_CHECK(s.has_value(), name, " is required for this optimizer");
    TORCH_CHECK(s->is_cuda() && s->scalar_type() == torch::kFloat32 &&
                    s->is_contiguous() && (size_t)s->numel() == n,
                name, " must match p");
    return s->data_ptr<float>();
  };
  bf16* plp_ptr = nullptr;
  if (plp.has_value()) {
    TORCH_CHECK(plp->is_cuda() && plp->scalar_type() == torch::kBFloat16 &&
                    plp->is_contiguous() && (size_t)plp->numel() == n,
                "p_lp must be a bf16 mirror of p");
    plp_ptr = (bf16*)plp->data_ptr();
  }
  float h0 = (float)hyper[0], h1 = (float)hyper[1], h2 = (float)hyper[2],
        h3 = (float)hyper[3];
  float *a = nullptr, *b = nullptr, *c = nullptr;
  switch (kind) {
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
  hipLaunchKernelGGL(opt_bump_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     step_buf.data_ptr<int>());
  gordo_masked::note_optimizer_launch("opt", false);
  if (n == 0) return;
  int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
#define GORDO_OPT_LAUNCH(K)                                                  \
  hipLaunchKernelGGL(opt_kernel<K>, dim3(blocks), dim3(256), 0,              \
                     cur_stream(), p.data_ptr<float>(), g.data_ptr<float>(), \
                     a, b, c, plp_ptr, n, h0, h1, h2, h3, flag ? 1 : 0,      \
                     step_buf.data_ptr<int>())
  switch (kind) {
    case OPT_SGD: GORDO_OPT_LAUNCH(OPT_SGD); break;
    case OPT_RMSPROP: GORDO_OPT_LAUNCH(OPT_RMSPROP); break;
    case OPT_ADAGRAD: GORDO_OPT_LAUNCH(OPT_ADAGRAD); break;
    case OPT_ADAM_AMSGRAD: GORDO_OPT_LAUNCH(OPT_ADAM_AMSGRAD); break;
    default: GORDO_OPT_LAUNCH(OPT_ADAMAX); break;
  }
#undef GORDO_OPT_LAUNCH
}

}  // namespace gordo_train
