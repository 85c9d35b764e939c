// The group-lasso penalty of the reference's training drivers (QViT_with_GETA/utils.py:157-194, called at :283-287
// before backward() and grad_clipping()) and the per-unit weights it reads (gl_scale,
// base_hybrid_sparse_optimizer.py:293-333), over the pruning tables of prune_step.hip:
//   qvit_group_lasso        sumsq[u] = sum p^2 of unit u over its members, coef[u] = lambda scale_u / sqrt(sumsq[u]),
//                           grad += coef[u] p in place on every member that has a gradient, and
//                           loss = sum_u scale_u sqrt(sumsq[u]);
//   qvit_group_lasso_scale  scale_u from the saliency scores of a period boundary.
// p is read from memory once where a unit is one row, m and v are never touched, and there are no atomics: every
// sum is a lane-strided double accumulation, the wave tree, and a fold in a fixed order.
//
// One-row units (the MLP groups) take a single pass. A wave owns a unit across its members and keeps the unit in
// registers: kSlots float4 per lane, a slot being 256 consecutive elements of one member (64 float4 of a member on
// the 16-byte path, 4 x 64 single elements of any other, loaded by the same lanes). The unit's slots are dealt member
// after member by a wave-uniform cursor inside a fully unrolled loop, so every slot is a named register. The wave
// sums p^2 from the registers, forms coef, and does the gradient's read-modify-write from them. A unit that needs
// more than kSlots slots streams instead: it sums from memory and reads p again for the gradient.
//
// Units of several rows (heads) are few and large (144 units of 0.6 MB on ViT-B), so a workgroup per unit would leave
// most CUs idle. Their rows are the work: a wave per row sums p^2 (group_lasso_rows_kernel), a wave per unit adds its
// rows' sums, listed section-major, rows ascending (qvit_prune_scores_fold's order), and forms coef, and a wave per
// row adds the gradient, reading p a second time.
#include <cmath>

#include "prune_common.h"

namespace {

constexpr int kSlots = QVIT_GROUP_LASSO_SLOTS;   // float4 per lane a unit may hold: 32 VGPRs
constexpr int kSlotElems = 64 * kVec;            // elements of one member per slot

// the penalised gradient of one element; every path, vector or scalar, held or streamed, goes through it
QVIT_DEV float penalised(float g, float p, float coef) {
#pragma clang fp contract(off)
  return g + coef * p;
}

QVIT_DEV double square(float p) { return (double)p * (double)p; }

// lambda scale / ||unit||, 0 for a unit of norm 0 (torch.norm's backward gives 0 there): no division, no NaN
QVIT_DEV float unit_coef(double sumsq, const float* scale, int64_t u, double lambda) {
  if (sumsq == 0.0) return 0.f;
  return (float)(lambda * (double)(scale ? scale[u] : 1.f) / sqrt(sumsq));
}

QVIT_DEV int64_t member_slots(const PruneMember& t) { return t.p ? (t.width + kSlotElems - 1) / kSlotElems : 0; }

// slot c of row `p` of a member: zeros past the row's end, which add nothing to the sum
QVIT_DEV float4 load_slot(const float* __restrict__ p, bool vec, int64_t width, int64_t c, int lane) {
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    const int64_t i = c * 64 + lane;
    if (i < width / kVec) q = reinterpret_cast<const float4*>(p)[i];
  } else {
    const int64_t e = c * kSlotElems + lane;
    if (e < width) q.x = p[e];
    if (e + 64 < width) q.y = p[e + 64];
    if (e + 128 < width) q.z = p[e + 128];
    if (e + 192 < width) q.w = p[e + 192];
  }
  return q;
}

QVIT_DEV void add_slot(float* __restrict__ g, bool vec, int64_t width, int64_t c, int lane, const float4& q,
                       float coef) {
  if (vec) {
    const int64_t i = c * 64 + lane;
    if (i >= width / kVec) return;
    float4 g4 = reinterpret_cast<const float4*>(g)[i];
    g4.x = penalised(g4.x, q.x, coef);
    g4.y = penalised(g4.y, q.y, coef);
    g4.z = penalised(g4.z, q.z, coef);
    g4.w = penalised(g4.w, q.w, coef);
    reinterpret_cast<float4*>(g)[i] = g4;
  } else {
    const int64_t e = c * kSlotElems + lane;
    if (e < width) g[e] = penalised(g[e], q.x, coef);
    if (e + 64 < width) g[e + 64] = penalised(g[e + 64], q.y, coef);
    if (e + 128 < width) g[e + 128] = penalised(g[e + 128], q.z, coef);
    if (e + 192 < width) g[e + 192] = penalised(g[e + 192], q.w, coef);
  }
}

// f(s, member, c) for the slots s = 0, 1, .. of a unit in turn: slot c of one member after another. The loop is
// unrolled, so s is a constant in every call and a register array indexed by it stays in registers; the cursor
// (k, c) is wave-uniform.
template <typename F>
QVIT_DEV void for_slots(const PruneGroup& G, const PruneMember* __restrict__ members, F f) {
  int k = 0;
  int64_t c = 0;
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    while (k < G.member_count && c >= member_slots(members[G.member_begin + k])) {
      ++k;
      c = 0;
    }
    if (k >= G.member_count) break;
    f(s, members[G.member_begin + k], c);
    ++c;
  }
}

// the lane's part of sum p^2 over row `row` of member t, from memory
QVIT_DEV double row_sumsq(const PruneMember& t, int64_t row, int lane) {
  const float* __restrict__ p = t.p + row * t.width;
  const int64_t nv = member_vec(t) ? t.width / kVec : 0;
  double s = 0.0;
  for (int64_t i = lane; i < nv; i += 64) {
    const float4 q = reinterpret_cast<const float4*>(p)[i];
    s += square(q.x);
    s += square(q.y);
    s += square(q.z);
    s += square(q.w);
  }
  for (int64_t i = nv * kVec + lane; i < t.width; i += 64) s += square(p[i]);
  return s;
}

// grad += coef p over row `row` of member t (which has a gradient), p from memory
QVIT_DEV void row_add(const PruneMember& t, int64_t row, int lane, float coef) {
  const float* __restrict__ p = t.p + row * t.width;
  float* __restrict__ g = const_cast<float*>(t.grad) + row * t.width;
  const int64_t nv = member_vec(t) ? t.width / kVec : 0;
  for (int64_t i = lane; i < nv; i += 64) {
    const float4 q = reinterpret_cast<const float4*>(p)[i];
    float4 g4 = reinterpret_cast<const float4*>(g)[i];
    g4.x = penalised(g4.x, q.x, coef);
    g4.y = penalised(g4.y, q.y, coef);
    g4.z = penalised(g4.z, q.z, coef);
    g4.w = penalised(g4.w, q.w, coef);
    reinterpret_cast<float4*>(g)[i] = g4;
  }
  for (int64_t i = nv * kVec + lane; i < t.width; i += 64) g[i] = penalised(g[i], p[i], coef);
}

// ---- one-row units: norm, coef and gradient in one pass, the unit held in registers ---------------------------------
__global__ __launch_bounds__(kThreads) void group_lasso_unit_kernel(const PruneGroup* __restrict__ groups, int ngroups,
                                                                    const PruneMember* __restrict__ members,
                                                                    int nmembers, const PruneItem* __restrict__ units,
                                                                    int64_t nunits, const float* __restrict__ scale,
                                                                    double lambda, double* __restrict__ sumsq,
                                                                    float* __restrict__ coef) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + wave; u < nunits; u += (int64_t)gridDim.x * kWaves) {
    const PruneItem un = units[u];
    PruneGroup G;
    const bool ok = item_group(un, groups, ngroups, nmembers, G);
    if (ok && rows_per_unit(G) > 1) continue;   // the fold kernel's unit
    float4 reg[kSlots];
    bool held = false;
    double ss = 0.0;
    if (ok) {
      int64_t need = 0;
      for (int k = 0; k < G.member_count; ++k) need += member_slots(members[G.member_begin + k]);
      held = need <= kSlots;
      if (held) {
        for_slots(G, members, [&](int s, const PruneMember& t, int64_t c) {
          reg[s] = load_slot(t.p + (int64_t)un.row * t.width, member_vec(t), t.width, c, lane);
          ss += square(reg[s].x);
          ss += square(reg[s].y);
          ss += square(reg[s].z);
          ss += square(reg[s].w);
        });
      } else {
        for (int k = 0; k < G.member_count; ++k) {
          const PruneMember t = members[G.member_begin + k];
          if (t.p) ss += row_sumsq(t, un.row, lane);
        }
      }
    }
    ss = __shfl(wave_sum(ss), 0, 64);
    const float c = unit_coef(ss, scale, u, lambda);
    if (lane == 0) {
      sumsq[u] = ss;
      coef[u] = c;
    }
    if (c == 0.f) continue;   // a zeroed unit, or lambda == 0: the gradient keeps its bits
    if (held) {
      for_slots(G, members, [&](int s, const PruneMember& t, int64_t cc) {
        if (t.grad)
          add_slot(const_cast<float*>(t.grad) + (int64_t)un.row * t.width, member_vec(t), t.width, cc, lane, reg[s],
                   c);
      });
    } else {
      for (int k = 0; k < G.member_count; ++k) {
        const PruneMember t = members[G.member_begin + k];
        if (t.p && t.grad) row_add(t, un.row, lane, c);
      }
    }
  }
}

// ---- units of several rows: a wave per row ------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void group_lasso_rows_kernel(const PruneGroup* __restrict__ groups, int ngroups,
                                                                    const PruneMember* __restrict__ members,
                                                                    int nmembers, const PruneItem* __restrict__ rows,
                                                                    int64_t nrows, double* __restrict__ rowsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < nrows; i += (int64_t)gridDim.x * kWaves) {
    const PruneItem it = rows[i];
    PruneGroup G;
    double s = 0.0;
    if (item_group(it, groups, ngroups, nmembers, G)) {
      for (int k = 0; k < G.member_count; ++k) {
        const PruneMember t = members[G.member_begin + k];
        if (t.p) s += row_sumsq(t, it.row, lane);
      }
    }
    s = wave_sum(s);
    if (lane == 0) rowsum[i] = s;
  }
}

// a wave per unit of several rows: lane l adds the sums of the unit's rows l, l + 64, .. as `rows` lists them
// (section-major, rows ascending), then the wave tree; lane 0 forms coef. A unit whose rows do not agree with the
// tables (their group, row and unit are compared) gets zeros. One wave and not one thread: a thread's 192 dependent
// loads took longer than the whole gradient pass. The grid is not capped: most units are one-row and leave at once.
__global__ __launch_bounds__(kThreads) void group_lasso_fold_kernel(const PruneGroup* __restrict__ groups, int ngroups,
                                                                    int nmembers, const PruneItem* __restrict__ units,
                                                                    int64_t nunits, const PruneItem* __restrict__ rows,
                                                                    int64_t nrows, const double* __restrict__ rowsum,
                                                                    const float* __restrict__ scale, double lambda,
                                                                    double* __restrict__ sumsq,
                                                                    float* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (u >= nunits) return;
  const PruneItem un = units[u];
  PruneGroup G;
  if (!item_group(un, groups, ngroups, nmembers, G) || rows_per_unit(G) <= 1) return;   // the unit kernel's
  const int64_t S = G.sections > 1 ? G.sections : 1, R = G.unit_rows > 1 ? G.unit_rows : 1;
  const int64_t count = G.rows / (S * R), base = un.link, h = un.row;
  const bool inside = count * S * R == G.rows && h < count && base >= 0 && base + S * R <= nrows;
  bool bad = false;
  double ss = 0.0;
  for (int64_t i = lane; inside && i < S * R; i += 64) {
    const int64_t s = i / R, j = i - s * R;
    const PruneItem it = rows[base + i];
    if (it.group != un.group || it.row != (s * count + h) * R + j || it.link != u) bad = true;
    else ss += rowsum[base + i];
  }
  ss = wave_sum(ss);
  const bool ok = inside && !__any(bad);
  if (lane != 0) return;
  if (!ok) ss = 0.0;
  sumsq[u] = ss;
  coef[u] = unit_coef(ss, scale, u, lambda);
}

__global__ __launch_bounds__(kThreads) void group_lasso_rows_add_kernel(const PruneGroup* __restrict__ groups,
                                                                        int ngroups,
                                                                        const PruneMember* __restrict__ members,
                                                                        int nmembers,
                                                                        const PruneItem* __restrict__ rows,
                                                                        int64_t nrows, int64_t nunits,
                                                                        const float* __restrict__ coef) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < nrows; i += (int64_t)gridDim.x * kWaves) {
    const PruneItem it = rows[i];
    PruneGroup G;
    if (!item_group(it, groups, ngroups, nmembers, G) || (uint32_t)it.link >= (uint64_t)nunits) continue;
    const float c = coef[it.link];
    if (c == 0.f) continue;
    for (int k = 0; k < G.member_count; ++k) {
      const PruneMember t = members[G.member_begin + k];
      if (t.p && t.grad) row_add(t, it.row, lane, c);
    }
  }
}

// ---- the penalty's value: one block of 1024, thread i adds units i, i + 1024, .. in that order, then the wave tree
// and the waves in index order
constexpr int kLossThreads = 1024;
__global__ __launch_bounds__(kLossThreads) void group_lasso_loss_kernel(const double* __restrict__ sumsq,
                                                                        int64_t nunits,
                                                                        const float* __restrict__ scale,
                                                                        float* __restrict__ loss) {
  __shared__ double lds[kLossThreads / 64];
  double s = 0.0;
#pragma unroll 4
  for (int64_t u = threadIdx.x; u < nunits; u += kLossThreads)
    s += (double)(scale ? scale[u] : 1.f) * sqrt(sumsq[u]);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = lds[0];
  for (int w = 1; w < kLossThreads / 64; ++w) s += lds[w];
  loss[0] = (float)s;
}

// ---- gl_scale: one block, in double -----------------------------------------------------------------------------
// clamp(group_cost^0.5 / max(|score|, 1e-8), 0.1, 10), then nan_to_num: a NaN score gives 1 (the clamp has already
// taken the infinities to its bounds). A unit that names no group counts as 1.
QVIT_DEV double inverse_score(const PruneItem& un, const PruneGroup* groups, int ngroups, float score) {
  if ((uint32_t)un.group >= (uint32_t)ngroups) return 1.0;
  const int64_t elems = groups[un.group].elems;
  const double a = fabs((double)score);
  double inv = sqrt((double)(elems > 1 ? elems : 1)) / (a < 1e-8 ? 1e-8 : a);   // a NaN score stays NaN
  inv = inv < 0.1 ? 0.1 : (inv > 10.0 ? 10.0 : inv);
  return inv != inv ? 1.0 : inv;
}

__global__ __launch_bounds__(kThreads) void group_lasso_scale_kernel(const PruneGroup* __restrict__ groups,
                                                                     int ngroups, const PruneItem* __restrict__ units,
                                                                     int64_t nunits, const float* __restrict__ scores,
                                                                     float* __restrict__ scale) {
  __shared__ double lds[kWaves][3];
  __shared__ double mean;
  double s = 0.0, unused1 = 0.0, unused2 = 0.0;
  for (int64_t u = threadIdx.x; u < nunits; u += kThreads) s += inverse_score(units[u], groups, ngroups, scores[u]);
  block_sum3(s, unused1, unused2, lds);
  if (threadIdx.x == 0) {
    const double m = s / (double)nunits;
    mean = m < 1e-8 ? 1e-8 : m;
  }
  __syncthreads();
  for (int64_t u = threadIdx.x; u < nunits; u += kThreads)
    scale[u] = (float)(inverse_score(units[u], groups, ngroups, scores[u]) / mean);
}

inline dim3 wave_grid(int64_t n) {
  const int64_t g = cdiv(n, kWaves);
  return dim3((unsigned)(g < 1 ? 1 : (g < kGridCap ? g : kGridCap)));
}

}  // namespace

extern "C" {

int qvit_group_lasso(const void* groups, int ngroups, const void* members, int nmembers, const void* units,
                     int64_t nunits, const void* rows, int64_t nrows, const float* scale, double lambda, double* sumsq,
                     float* coef, float* loss, hipStream_t stream) {
  if (!groups || !members || !units || !sumsq || !coef || !loss || (nrows > 0 && !rows)) return QVIT_ENULL;
  if (qvit_misaligned(7, groups, members, units, rows, sumsq) || qvit_misaligned(3, scale, coef, loss))
    return QVIT_EALIGN;
  if (ngroups < 0 || nmembers < 0 || nunits < 0 || nunits > INT32_MAX || nrows < 0 || nrows > INT32_MAX)
    return QVIT_EINVAL;
  if (!std::isfinite(lambda) || lambda < 0.0) return QVIT_EINVAL;
  if (ngroups == 0 || nmembers == 0 || nunits == 0) return QVIT_OK;
  const PruneGroup* G = static_cast<const PruneGroup*>(groups);
  const PruneMember* M = static_cast<const PruneMember*>(members);
  const PruneItem* U = static_cast<const PruneItem*>(units);
  const PruneItem* R = static_cast<const PruneItem*>(rows);
  double* rowsum = sumsq + nunits;
  hipLaunchKernelGGL(group_lasso_unit_kernel, wave_grid(nunits), dim3(kThreads), 0, stream, G, ngroups, M, nmembers,
                     U, nunits, scale, lambda, sumsq, coef);
  if (nrows > 0) {
    hipLaunchKernelGGL(group_lasso_rows_kernel, wave_grid(nrows), dim3(kThreads), 0, stream, G, ngroups, M, nmembers,
                       R, nrows, rowsum);
    hipLaunchKernelGGL(group_lasso_fold_kernel, dim3((unsigned)cdiv(nunits, kWaves)), dim3(kThreads), 0, stream, G,
                       ngroups, nmembers, U, nunits, R, nrows, rowsum, scale, lambda, sumsq, coef);
    hipLaunchKernelGGL(group_lasso_rows_add_kernel, wave_grid(nrows), dim3(kThreads), 0, stream, G, ngroups, M,
                       nmembers, R, nrows, nunits, coef);
  }
  hipLaunchKernelGGL(group_lasso_loss_kernel, dim3(1), dim3(kLossThreads), 0, stream, sumsq, nunits, scale, loss);
  return qvit_launch_status();
}

int qvit_group_lasso_scale(const void* groups, int ngroups, const void* units, int64_t nunits, const float* scores,
                           float* scale, hipStream_t stream) {
  if (!groups || !units || !scores || !scale) return QVIT_ENULL;
  if (qvit_misaligned(7, groups, units) || qvit_misaligned(3, scores, scale)) return QVIT_EALIGN;
  if (ngroups < 0 || nunits < 0 || nunits > INT32_MAX) return QVIT_EINVAL;
  if (ngroups == 0 || nunits == 0) return QVIT_OK;
  hipLaunchKernelGGL(group_lasso_scale_kernel, dim3(1), dim3(kThreads), 0, stream,
                     static_cast<const PruneGroup*>(groups), ngroups, static_cast<const PruneItem*>(units), nunits,
                     scores, scale);
  return qvit_launch_status();
}

}  // extern "C"
