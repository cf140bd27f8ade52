// Host-only planner of the grouped LayerNormalization launches
// (layernorm.hip): how many lanes own a row, whether the 16-byte arm runs,
// how the rows of a model are split into chunks and on how many
// workgroups. The launchers launch the plan they get, the launch record is
// the plan, and Python asks it (ops.layer_norm_plan,
// ops.layer_norm_refusal). Plain C++17, no torch / HIP / device call.
#pragma once

#include <string>

namespace gordo_ln {

constexpr int THREADS = 256;   // four waves per workgroup
constexpr int CHUNK = 8;       // bf16 per lane: one 16-byte load
constexpr int MAX_FP = 512;    // 64 lanes x 8 columns
// backward grid target: about two workgroups per CU, the figure
// grouped_wgrad_pipe_kernel and the Conv1D kernels aim for
constexpr int TARGET_WGS = 512;

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// lanes that own one row: the power of two >= ceil(Fp / 8), at least 4
inline int lanes_for(int Fp) {
  int L = 4;
  while (L * CHUNK < Fp) L *= 2;
  return L;
}

// What to launch. A refusal carries its message in `error` and nothing
// else. Forward: one workgroup per `rows_per_block` rows of one model
// (chunks = row groups of a model). Backward: a workgroup walks
// `passes` row groups of one model, chunks of them per model; the
// partial parameter gradients are [G, chunks, 2, Fp].
struct LnPlan {
  bool fwd = true;
  int lanes = 0;
  bool vec = false;  // set by the launcher (alignment is a runtime fact)
  int rows_per_block = 0;
  int passes = 0;
  int chunks = 0, blocks = 0;
  std::string error;
  bool ok() const { return error.empty(); }
  const char* family_name() const { return fwd ? "ln_fwd" : "ln_bwd"; }
};

inline LnPlan refuse_ln(std::string msg) {
  LnPlan p;
  p.error = std::move(msg);
  return p;
}

inline LnPlan plan_layer_norm(bool fwd, int G, int B, int Fp) {
  if (G < 1 || B < 1 || Fp < 1)
    return refuse_ln("LayerNormalization needs G, B, Fp >= 1");
  if (Fp > MAX_FP)
    return refuse_ln(
        "LayerNormalization needs a padded width Fp <= 512 (one 16-byte "
        "chunk per lane of a wave), got Fp = " + std::to_string(Fp));
  LnPlan p;
  p.fwd = fwd;
  p.lanes = lanes_for(Fp);
  p.rows_per_block = THREADS / p.lanes;
  const int groups = ceil_div(B, p.rows_per_block);
  if (fwd) {
    p.passes = 1;
    p.chunks = groups;
  } else {
    // about one resident wave of workgroups over all models
    const int target = TARGET_WGS / G > 1 ? TARGET_WGS / G : 1;
    p.passes = ceil_div(groups, target < groups ? target : groups);
    p.chunks = ceil_div(groups, p.passes);
  }
  if (p.chunks > 65535)
    return refuse_ln("LayerNormalization: too many row groups in one launch, "
                     "B = " + std::to_string(B));
  p.blocks = G * p.chunks;
  return p;
}

}  // namespace gordo_ln
