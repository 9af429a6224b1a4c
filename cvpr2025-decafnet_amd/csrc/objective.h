// Point annotation and the Trainer's fused objective (objective.hip): parameter blocks shared by the two kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcf {

constexpr int OBJ_MAX_LEVELS = 16;

// The candidate points of PtGenerator (libs/modeling/model.py:668-743) as a rule instead of a table: point i of a row lies on the
// level l with off[l] <= i < off[l + 1], its stride is 2^l, its coordinate (i - off[l]) * 2^l (+ 2^l - 0.5 with use_offset, see level_ctx), and its
// regression range [lo[l], hi[l]) is the table PtGenerator.__init__ derives (model.py:686-696), rounded to fp32 as the buffer is.
struct PointRule {
  int T, L, S;                          // level-0 length, levels, points per row (sum_l T >> l)
  int off[OBJ_MAX_LEVELS + 1];
  float lo[OBJ_MAX_LEVELS], hi[OBJ_MAX_LEVELS];
  int use_offset;
  int radius_sampling;                  // 1: centre sampling inside `radius` strides of the segment centre; 0: inside the segment
  float radius;                         // center_sampling_radius as fp32 (the reference multiplies an fp32 tensor by it)
};

// fills `r` (false: T, L or the range parameters are not a PtGenerator's)
bool make_point_rule(PointRule& r, int64_t T, int L, double regression_range, double sigma, int use_offset, int64_t max_seq_len,
                     int center_sampling, double radius);

struct AnnotateArgs {
  PointRule rule;
  const float* targets;                 // [nrows][2]
  uint8_t* labels;                      // [nrows][S]
  float* offsets;                       // [nrows][S][2]
  uint8_t* in_window;                   // [nrows][S] or nullptr
  uint8_t* in_range;                    // [nrows][S] or nullptr
};

struct ObjectiveArgs {
  PointRule rule;
  const float* logits1;                 // [nrows][S] or nullptr (one classification head)
  const float* logits2;                 // [nrows][S]
  const float* offsets;                 // [nrows][S][2]
  const uint8_t* masks;                 // [nrows][S]
  const float* targets;                 // [nrows][2]
  int vec;                              // 1: S % 4 == 0 and every pointer is 16-byte aligned -> 4 points per load
  float alpha, t_pos, t_neg, eps;       // focal alpha; the smoothed label of a positive / negative point
  int kind;                             // 0 GIoU, 1 DIoU
  int bpr;                              // workgroups per row, a function of S alone
  float* part;                          // [nrows][bpr][4] scratch
};

// Gradient side of k_objective: d total / d (logits1, logits2, offsets), times the upstream gradients
struct ObjectiveGradArgs {
  float* g_logits1;                     // [nrows][S] or nullptr (with logits1)
  float* g_logits2;                     // [nrows][S]
  float* g_offsets;                     // [nrows][S][2]
  const float* loss_norm;               // device scalar
  const float* grad_total;              // device scalar: upstream gradient of `total`, nullptr = 1
  const float* grad_parts;              // device float[2]: upstream gradients of `cls` and `reg` on their own, nullptr = 0
  float world_size, loss_weight;
  int accumulate;                       // 1: add into the g_* buffers instead of overwriting them
};

int launch_annotate(const AnnotateArgs& a, int nrows, hipStream_t st);
// bytes of scratch launch_objective needs for (nrows, S): the partials and the row results
size_t objective_scratch_bytes(int nrows, int S);
int objective_blocks_per_row(int S);
int launch_objective(const ObjectiveArgs& a, int nrows, const float* loss_norm, float world_size, float loss_weight, float* rows_scratch,
                     float* rows_out, float* out4, hipStream_t st);
int launch_objective_grad(const ObjectiveArgs& a, const ObjectiveGradArgs& g, int nrows, float* rows_scratch, float* rows_out, float* out4,
                          hipStream_t st);

}  // namespace dcf
