// The pruning stages of the GETA optimizer for declared row groups (optimizer/geta.py:167-248 period boundary,
// :281-521 compute_gamma_d, :944-1022 the joint stage; base_hybrid_sparse_optimizer.py:194-211, :221-291;
// importance_score/*.py), as a fixed number of launches per step whatever the number of groups:
//   qvit_prune_scores / qvit_prune_scores_finish   the saliency scores of every row of every group (period boundary),
//   qvit_prune_scores_fold                         between them where a group's unit is a set of rows;
//   qvit_prune_joint_scalars                       the quantizer scalars of the joint groups' layers;
//   qvit_prune_joint_reduce / _finish              the six sums of compute_gamma_d, then gamma and d per group;
//   qvit_prune_joint_apply                         the member tensors' update, moments and row zeroing.
// Nothing is read back and nothing waits on data: the reference's `while d_quant < d_quant_lower` is an iteration
// cap here (kLoopCap).
//
// A group is a set of member tensors sliced along dim 0 (the reference's TensorTransform.BASIC): row r of the group
// is row r of every member. The host keeps three device tables: PruneGroup (64 B), PruneMember (48 B, QatTensor's
// layout with the row width where that has numel) and PruneItem (16 B) = (group, row, state). Every streaming kernel
// deals items to waves: a wave owns one row of one group across all its members, so a row's sums need no partials
// and no atomics. A member whose four base pointers are 16-byte aligned and whose width is a multiple of 4 is read
// and written 16 bytes at a time; any other member one element at a time, by the same per-element function.
//
// A group with sections > 1 or unit_rows > 1 prunes units of sections x unit_rows rows: unit h of a member of
// sections x units x unit_rows rows is the rows (s units + h) unit_rows + j (head h of a qkv projection: sections = 3,
// unit_rows = the head dim). The rows stay the items and the waves' work, so nothing above changes: the host gives
// every row its unit's state, lists a redundant unit's rows in the reduce, and only the scores need the unit: one
// thread per unit folds its rows' three sums in a fixed order (qvit_prune_scores_fold) before the criteria are formed.
//
// The gradient variant is recomputed in registers from grad, m and v by qat_common.h's grad_variant, the function
// the dense step runs, so no grad_variant tensor exists and a member row outside the redundant set gets the bits
// qvit_qat_step would give it (minus adamw's decay in the joint branch, as in the reference). Sums are double, in a
// fixed order: lane-strided accumulation, the wave tree, then (joint finish) partials folded in index order.
#include "qat_common.h"

namespace {

constexpr int kLoopCap = 861;   // ceil(ln(FLT_MAX / FLT_TRUE_MIN) / ln(1.25)): x 1.25 per turn crosses fp32's range

struct PruneMember {    // 48 B
  float* p;
  const float* grad;    // NULL: no update (pruned rows are still zeroed), no part in the sums
  float* m;
  float* v;
  int64_t width;        // elements per row
  int32_t quantized;    // 1: the group's layer's weight (clip, res and quantize by its weight quantizer)
  int32_t flags;        // bit 0: this tensor's first step
};
struct PruneGroup {     // 64 B
  float* d;             // weight quantizer scalars of the group's layer; t NULL: the linear type
  const float* qm;
  const float* t;
  int32_t member_begin, member_count;
  int32_t rows;
  int32_t joint;        // 1: the joint stage (active redundant rows); 0: the stage path
  int32_t red_begin, red_count;   // its redundant rows' partials
  int64_t elems;        // elements per unit over all members
  int32_t sections, unit_rows;    // 0 as 1; both 1: a unit is one row
};
struct PruneItem {      // 16 B
  int32_t group, row;
  int32_t state;        // 0 important, 1 active redundant, 2 pruned
  int32_t link;         // a row item: the row's unit (0 where a unit is one row); a unit entry of the fold (row = the
                        // unit): the index in the row items of row 0 of its group
};
enum { kImportant = 0, kRedundant = 1, kPruned = 2 };
QVIT_DEV int64_t rows_per_unit(const PruneGroup& G) {
  return (int64_t)(G.sections > 1 ? G.sections : 1) * (G.unit_rows > 1 ? G.unit_rows : 1);
}

// the weight quantizer as geta.py:806-850 states it: range_pow has no 1e-6 (the layers' forward has one)
struct WeightQuant {
  bool nonlinear;
  float d, qm, t, rp;
  QParams qp;   // for quant_code_from_pow: d, qm, L
};
QVIT_DEV WeightQuant load_weight_quant(const PruneGroup& G) {
  WeightQuant w;
  w.nonlinear = G.t != nullptr;
  w.d = *G.d;
  w.qm = *G.qm;
  w.t = w.nonlinear ? *G.t : 1.f;
  const float aq = fabsf(w.qm);
  w.rp = w.nonlinear ? exp_cr(w.t * log_cr(aq)) : aq;
  w.qp.qtype = w.nonlinear ? QVIT_QT_NONLINEAR : QVIT_QT_LINEAR;
  w.qp.careful = 1; w.qp.d = w.d; w.qp.inv_d = 1.f / w.d; w.qp.qm = w.qm; w.qp.t = w.t; w.qp.levels = 0.f;
  w.qp.L = rintf(w.rp / w.d);
  return w;
}
QVIT_DEV float pow_abs(float a, const WeightQuant& w) { return w.nonlinear ? exp_cr(w.t * log_cr(a)) : a; }
QVIT_DEV float with_sign(float mag, float x) { return x > 0.f ? mag : (x < 0.f ? -mag : 0.f); }
// _clip_helper (:821-833) and _residual_helper (:835-850) of one element
QVIT_DEV void clip_res(float x, const WeightQuant& w, float& clip, float& res) {
#pragma clang fp contract(off)
  const float a = fabsf(x);
  const float pw = (a >= w.qm) ? w.rp : pow_abs(a, w);
  const float q = pw / w.d;
  clip = with_sign(pw, x);
  res = with_sign(rintf(q) - q, x);
}
// _quantize_helper (:806-819) of one element: d * code, by qvit_common.h's careful sequence
QVIT_DEV float quantize_weight(float x, const WeightQuant& w) {
  return w.qp.d * quant_code_from_pow(x, pow_abs(fabsf(x), w), w.qp);
}

QVIT_DEV bool member_vec(const PruneMember& t) {
  return ((((uintptr_t)t.p | (uintptr_t)t.grad | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0) && (t.width & 3) == 0;
}

// Walks row `row` of member t: f(i, p, g, m, v) per element with m, v loaded (0 when fresh or absent); f returns the
// new p. WRITE stores p, m, v back. The vector and the scalar path call the same f.
template <int VARIANT, bool WRITE, typename F>
QVIT_DEV void walk_row(const PruneMember& t, int64_t row, int lane, const Hyper& h, F f) {
  const int64_t off = row * t.width;
  float* __restrict__ p = t.p + off;
  const float* __restrict__ g = t.grad + off;
  float* __restrict__ m = (t.m && h.mom1 > 0.f) ? t.m + off : nullptr;
  float* __restrict__ v = (t.v && VARIANT != QVIT_QAT_SGD && h.mom2 > 0.f) ? t.v + off : nullptr;
  const bool fresh = h.first_step || (t.flags & 1);
  const int64_t nv = member_vec(t) ? t.width / kVec : 0;
  for (int64_t i = lane; i < nv; i += 64) {
    float4 p4 = reinterpret_cast<const float4*>(p)[i];
    const float4 g4 = reinterpret_cast<const float4*>(g)[i];
    float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
    if (m && !fresh) m4 = reinterpret_cast<const float4*>(m)[i];
    if (v && !fresh) v4 = reinterpret_cast<const float4*>(v)[i];
    p4.x = f(p4.x, g4.x, m4.x, v4.x, fresh);
    p4.y = f(p4.y, g4.y, m4.y, v4.y, fresh);
    p4.z = f(p4.z, g4.z, m4.z, v4.z, fresh);
    p4.w = f(p4.w, g4.w, m4.w, v4.w, fresh);
    if (WRITE) {
      reinterpret_cast<float4*>(p)[i] = p4;
      if (m) reinterpret_cast<float4*>(m)[i] = m4;
      if (v) reinterpret_cast<float4*>(v)[i] = v4;
    }
  }
  for (int64_t i = nv * kVec + lane; i < t.width; i += 64) {
    float mi = 0.f, vi = 0.f;
    if (m && !fresh) mi = m[i];
    if (v && !fresh) vi = v[i];
    const float pi = f(p[i], g[i], mi, vi, fresh);
    if (WRITE) {
      p[i] = pi;
      if (m) m[i] = mi;
      if (v) v[i] = vi;
    }
  }
}

// an item's group, checked against the tables; false: the item is skipped
QVIT_DEV bool item_group(const PruneItem& it, const PruneGroup* groups, int ngroups, int nmembers, PruneGroup& G) {
  if ((uint32_t)it.group >= (uint32_t)ngroups) return false;
  G = groups[it.group];
  return (uint32_t)it.row < (uint32_t)G.rows && G.member_begin >= 0 && G.member_count >= 0 &&
         (int64_t)G.member_begin + G.member_count <= nmembers;
}

// ---- scores: per row sum p^2, sum g^2, sum p g over the members (importance_score/*.py) ---------------------------
template <int VARIANT>
__global__ __launch_bounds__(kThreads) void prune_scores_kernel(const PruneGroup* __restrict__ groups, int ngroups,
                                                                const PruneMember* __restrict__ members, int nmembers,
                                                                const PruneItem* __restrict__ items, int64_t nitems,
                                                                double* __restrict__ sums, Hyper h) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < nitems; i += (int64_t)gridDim.x * kWaves) {
    const PruneItem it = items[i];
    PruneGroup G;
    double pp = 0.0, gg = 0.0, pg = 0.0;
    if (item_group(it, groups, ngroups, nmembers, G)) {
      for (int k = 0; k < G.member_count; ++k) {
        const PruneMember t = members[G.member_begin + k];
        if (!t.p) continue;
        if (!t.grad) {   // no gradient this step: magnitude only (`p_name not in grad_variant: continue`)
          const float* p = t.p + (int64_t)it.row * t.width;
          for (int64_t e = lane; e < t.width; e += 64) pp += (double)p[e] * (double)p[e];
          continue;
        }
        walk_row<VARIANT, false>(t, it.row, lane, h, [&](float p, float g, float& m, float& v, bool fresh) {
          const float gv = grad_variant<VARIANT>(p, g, m, v, fresh, h);
          pp += (double)p * (double)p;
          gg += (double)gv * (double)gv;
          pg += (double)p * (double)gv;
          return p;
        });
      }
    }
    pp = wave_sum(pp); gg = wave_sum(gg); pg = wave_sum(pg);
    if (lane == 0) {
      sums[3 * i] = pp; sums[3 * i + 1] = gg; sums[3 * i + 2] = pg;
    }
  }
}

// ---- scores of units of several rows: one thread per unit adds its rows' sums, section-major, row ascending -----------
__global__ __launch_bounds__(kThreads) void prune_scores_fold_kernel(const PruneGroup* __restrict__ groups, int ngroups,
                                                                     const PruneItem* __restrict__ items,
                                                                     int64_t nitems, const double* __restrict__ sums,
                                                                     const PruneItem* __restrict__ units,
                                                                     int64_t nunits, double* __restrict__ unit_sums) {
  const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (u >= nunits) return;
  const PruneItem un = units[u];
  double pp = 0.0, gg = 0.0, pg = 0.0;
  if ((uint32_t)un.group < (uint32_t)ngroups) {
    const PruneGroup G = groups[un.group];
    const int64_t S = G.sections > 1 ? G.sections : 1, R = G.unit_rows > 1 ? G.unit_rows : 1;
    const int64_t count = G.rows > 0 ? G.rows / (S * R) : 0, base = un.link, h = un.row;
    // the unit and its group's rows lie inside the tables, and the row items are the ones the unit names
    bool ok = count * S * R == G.rows && h >= 0 && h < count && base >= 0 && base + G.rows <= nitems;
    for (int64_t s = 0; ok && s < S; ++s)
      for (int64_t j = 0; j < R; ++j) {
        const int64_t r = (s * count + h) * R + j;
        const PruneItem it = items[base + r];
        if (it.group != un.group || it.row != r || (S * R > 1 && it.link != h)) {
          ok = false;
          break;
        }
        const double* q = sums + 3 * (base + r);
        pp += q[0]; gg += q[1]; pg += q[2];
      }
    if (!ok) pp = gg = pg = 0.0;
  }
  unit_sums[3 * u] = pp; unit_sums[3 * u + 1] = gg; unit_sums[3 * u + 2] = pg;
}

// the five criteria of one row, in double: magnitude, avg_magnitude, cosine_similarity, taylor first and second order
QVIT_DEV void criteria(const double* s, double elems, double c[5]) {
  const double np = sqrt(s[0]), ng = sqrt(s[1]);
  c[0] = np;
  c[1] = np / (elems + 1e-6);
  c[2] = s[2] / (np + 1e-8) / (ng + 1e-8) + 1.0;
  c[3] = fabs(s[2]);
  c[4] = 0.5 * c[3] * c[3];
}

// one block: the normalisers sqrt(1e-8 + sum score^2) + 1e-8 per criterion over all rows of all groups, then the
// weighted sum (base_hybrid_sparse_optimizer.py:230-271), in the order magnitude .. taylor_second_order
__global__ __launch_bounds__(kThreads) void prune_scores_finish_kernel(const PruneGroup* __restrict__ groups,
                                                                       int ngroups,
                                                                       const PruneItem* __restrict__ items,
                                                                       int64_t nitems, const double* __restrict__ sums,
                                                                       double w0, double w1, double w2, double w3,
                                                                       double w4, float* __restrict__ scores) {
  __shared__ double lds[kWaves][3];
  __shared__ double denom[5];
  double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < nitems; i += kThreads) {
    const int g = items[i].group;
    if ((uint32_t)g >= (uint32_t)ngroups) continue;
    double c[5];
    criteria(sums + 3 * i, (double)groups[g].elems, c);
#pragma unroll
    for (int k = 0; k < 5; ++k) q[k] += c[k] * c[k];
  }
  block_sum3(q[0], q[1], q[2], lds);
  if (threadIdx.x == 0) {
    denom[0] = q[0]; denom[1] = q[1]; denom[2] = q[2];
  }
  __syncthreads();
  double unused = 0.0;
  block_sum3(q[3], q[4], unused, lds);
  if (threadIdx.x == 0) {
    denom[3] = q[3]; denom[4] = q[4];
#pragma unroll
    for (int k = 0; k < 5; ++k) denom[k] = sqrt(1e-8 + denom[k]) + 1e-8;
  }
  __syncthreads();
  const double w[5] = {w0, w1, w2, w3, w4};
  for (int64_t i = threadIdx.x; i < nitems; i += kThreads) {
    const int g = items[i].group;
    if ((uint32_t)g >= (uint32_t)ngroups) {
      scores[i] = 0.f;
      continue;
    }
    double c[5], o = 0.0;
    criteria(sums + 3 * i, (double)groups[g].elems, c);
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (w[k] != 0.0) o += c[k] * (w[k] / denom[k]);
    scores[i] = (float)o;
  }
}

// ---- joint stage: the quantizer scalars of the joint groups' layers (geta.py:947-960) -----------------------------
// weight side: q_m and t step at lr_quant without decay, d is not stepped (the finish kernel writes it) but its
// moments move as compute_grad_variant moves them; activation side: the range stage's activation pass (:667-721).
template <int VARIANT>
__global__ __launch_bounds__(kThreads) void prune_joint_scalars_kernel(const QatQuant* __restrict__ quants,
                                                                       int nquants, Hyper h, int min_act,
                                                                       int max_act) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nquants) return;
  const QatQuant e = quants[i];
  if (!e.s[0] || !e.s[1] || !e.mom) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (!e.s[s] || !e.g[s]) continue;
    const bool fresh = h.first_step || ((e.flags >> s) & 1);
    float m = 0.f, v = 0.f;
    if (!fresh) {
      m = e.mom[s];
      v = e.mom[3 + s];
    }
    float p = *e.s[s];
    const float gv = grad_variant<VARIANT>(p, *e.g[s], m, v, fresh, h);
    if (e.side == 1) p = descend<VARIANT>(p, gv, h.lr_quant, h);
    else if (s != 0) p = fmaf(gv, -h.lr_quant, p);
    *e.s[s] = p;
    e.mom[s] = m;
    e.mom[3 + s] = v;
  }
  if (e.side != 1) return;
  const double qm = (double)*e.s[1], t = e.s[2] ? (double)*e.s[2] : 1.0;
  *e.s[0] = clamp_keep_nan(*e.s[0], (float)d_of_bits(max_act, qm, t), (float)d_of_bits(min_act, qm, t));
}

// ---- joint stage: <clip, g>, |clip|^2, |g|^2, <res, g>, |res|^2, sum clip per redundant row (geta.py:281-371) -----
template <int VARIANT>
__global__ __launch_bounds__(kThreads) void prune_joint_reduce_kernel(const PruneGroup* __restrict__ groups,
                                                                      int ngroups,
                                                                      const PruneMember* __restrict__ members,
                                                                      int nmembers,
                                                                      const PruneItem* __restrict__ items,
                                                                      int64_t nitems, double* __restrict__ partials,
                                                                      Hyper h) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < nitems; i += (int64_t)gridDim.x * kWaves) {
    const PruneItem it = items[i];
    PruneGroup G;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (item_group(it, groups, ngroups, nmembers, G) && G.d && G.qm) {
      const WeightQuant w = load_weight_quant(G);   // the stepped q_m and t, the old d
      for (int k = 0; k < G.member_count; ++k) {
        const PruneMember t = members[G.member_begin + k];
        if (!t.p || !t.grad) continue;
        const bool quantized = t.quantized != 0;
        walk_row<VARIANT, false>(t, it.row, lane, h, [&](float p, float g, float& m, float& v, bool fresh) {
          const float gv = grad_variant<VARIANT>(p, g, m, v, fresh, h);
          float clip = p, res = 0.f;
          if (quantized) clip_res(p, w, clip, res);
          s[0] += (double)clip * (double)gv;
          s[1] += (double)clip * (double)clip;
          s[2] += (double)gv * (double)gv;
          s[3] += (double)res * (double)gv;
          s[4] += (double)res * (double)res;
          s[5] += (double)clip;
          return p;
        });
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) partials[6 * i + k] = s[k];
    }
  }
}

// info word of a group's finish: bits 0..2 the gamma branch, the rest flags
enum {
  kGammaMeanZero = 0,      // mean(clip) < 1e-8
  kGammaNonFinite = 1,     // the cosine is inf or nan
  kGammaSchedule = 2,      // 0 <= cos <= 1
  kGammaNegative = 3,      // -1 <= cos < 0
  kGammaClampPos = 4,      // cos > 1, clamped: the schedule
  kGammaClampNeg = 5,      // cos < -1, clamped: the negative-cosine formula at -1
  kInfoDUpper = 1 << 3,    // cos_res >= 0 or gamma == 0: d = d_quant_upper
  kInfoLoop = 1 << 4,      // the x 0.8 loop ran at least once
  kInfoMin = 1 << 5,       // the final min took d_quant_upper
  kInfoCap = 1 << 6,       // the loop did not end within kLoopCap turns: d = d_quant_upper, gamma = 0
};

// one block per group: folds its rows' partials in index order, then thread 0 evaluates compute_gamma_d's scalar
// part (geta.py:373-499) in double
__global__ __launch_bounds__(kThreads) void prune_joint_finish_kernel(const PruneGroup* __restrict__ groups,
                                                                      int ngroups,
                                                                      const double* __restrict__ partials,
                                                                      int64_t npartials, double lr, int period,
                                                                      int t_in_period, int min_bit, int max_bit,
                                                                      float* __restrict__ gamma,
                                                                      int32_t* __restrict__ info) {
  __shared__ double lds[kWaves][3];
  const int g = blockIdx.x;
  if (g >= ngroups) return;
  const PruneGroup G = groups[g];
  const bool live = G.joint && G.red_count > 0 && G.red_begin >= 0 && G.d && G.qm &&
                    (int64_t)G.red_begin + G.red_count <= npartials;
  if (!live) {   // (uniform over the block)
    if (threadIdx.x == 0) {
      gamma[g] = 0.f;
      info[g] = -1;
    }
    return;
  }
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < G.red_count; j += kThreads) {
    const double* p = partials + 6 * ((int64_t)G.red_begin + j);
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += p[k];
  }
  block_sum3(s[0], s[1], s[2], lds);
  __syncthreads();
  block_sum3(s[3], s[4], s[5], lds);
  if (threadIdx.x != 0) return;

  const double eps = 1e-8, eta = 0.999, zeta = 0.9;
  const double clip_norm = sqrt(s[1]), grad_norm = sqrt(s[2]), res_norm = sqrt(s[4]);
  const double cos_clip = s[0] / (fmax(clip_norm, eps) * grad_norm);
  const double cos_res = s[3] / (fmax(res_norm, eps) * grad_norm);
  // red_count rows are red_count / rows_per_unit units of elems elements
  const double mean_clip = s[5] / ((double)(G.red_count / rows_per_unit(G)) * (double)G.elems);
  const double D = (double)period, tt = (double)t_in_period;
  const double schedule = 1.0 - (D - tt - 1.0) / (D - tt);
  double rate;
  int word;
  if (mean_clip < 1e-8) {   // the signed mean (:387)
    rate = 0.0; word = kGammaMeanZero;
  } else if (isinf(cos_clip) || isnan(cos_clip)) {
    rate = 0.0; word = kGammaNonFinite;
  } else if (cos_clip >= 0.0 && cos_clip <= 1.0) {
    rate = schedule; word = kGammaSchedule;
  } else if (cos_clip >= -1.0 && cos_clip < 0.0) {
    rate = -(1.0 - eta) * lr * grad_norm / (cos_clip * clip_norm); word = kGammaNegative;
  } else if (cos_clip > 1.0) {
    rate = schedule; word = kGammaClampPos;
  } else {
    rate = -(1.0 - eta) * lr * grad_norm / (-1.0 * clip_norm); word = kGammaClampNeg;
  }
  const double qm = (double)*G.qm, t = G.t ? (double)*G.t : 1.0;
  const double d_upper = d_of_bits(min_bit, qm, t), d_lower = d_of_bits(max_bit, qm, t);
  double d;
  if (cos_res >= 0.0 || rate == 0.0) {
    d = d_upper; word |= kInfoDUpper;
  } else {
    d = -zeta * eta * lr * grad_norm / (rate * cos_res * res_norm);
    int turns = 0;
    for (; turns < kLoopCap && d < d_lower; ++turns) {
      rate = rate * 0.8;
      d = d / 0.8;
    }
    if (turns) word |= kInfoLoop;
    if (d < d_lower) {   // the reference would loop for ever (d == 0): a zero gradient norm
      d = d_upper; rate = 0.0; word |= kInfoCap;
    } else if (!(d < d_upper)) {   // min(d_upper, d), which also takes d_upper for a NaN d
      d = d_upper; word |= kInfoMin;
    }
  }
  *G.d = (float)d;
  gamma[g] = (float)rate;
  info[g] = word;
}

// ---- the member tensors' update (geta.py:982-1008, :1022; the stage path for groups that are not joint) ----------
template <int VARIANT>
__global__ __launch_bounds__(kThreads) void prune_joint_apply_kernel(const PruneGroup* __restrict__ groups,
                                                                     int ngroups,
                                                                     const PruneMember* __restrict__ members,
                                                                     int nmembers,
                                                                     const PruneItem* __restrict__ items,
                                                                     int64_t nitems, const float* __restrict__ gamma,
                                                                     Hyper h) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < nitems; i += (int64_t)gridDim.x * kWaves) {
    const PruneItem it = items[i];
    PruneGroup G;
    if (!item_group(it, groups, ngroups, nmembers, G)) continue;
    const bool forget = G.joint && it.state == kRedundant && G.d && G.qm;
    const bool pruned = it.state == kPruned;
    const float rate = forget ? gamma[it.group] : 0.f;
    WeightQuant w;
    if (forget) w = load_weight_quant(G);   // the d the finish kernel wrote
    for (int k = 0; k < G.member_count; ++k) {
      const PruneMember t = members[G.member_begin + k];
      if (!t.p) continue;
      if (!t.grad) {
        if (pruned) {
          float* p = t.p + (int64_t)it.row * t.width;
          for (int64_t e = lane; e < t.width; e += 64) p[e] = 0.f;
        }
        continue;
      }
      const bool quantized = t.quantized != 0;
      walk_row<VARIANT, true>(t, it.row, lane, h, [&](float p, float g, float& m, float& v, bool fresh) {
#pragma clang fp contract(off)
        const float gv = grad_variant<VARIANT>(p, g, m, v, fresh, h);
        if (G.joint) {
          if (forget) p = p - rate * (quantized ? quantize_weight(p, w) : p);   // :990-1000
          p = fmaf(gv, -h.lr, p);                                               // :1008, no decay in this branch
        } else {
          p = descend<VARIANT>(p, gv, h.lr, h);
        }
        return pruned ? 0.f : p;   // fix_pruned_groups_as_zeros
      });
    }
  }
}

// the table checks the streaming entry points share, in the ABI's order
inline int tables_status(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                         int64_t nitems, const void* out) {
  if (!groups || !members || !items || !out) return QVIT_ENULL;
  if (qvit_misaligned(7, groups, members, items, out)) return QVIT_EALIGN;
  if (ngroups < 0 || nmembers < 0 || nitems < 0 || nitems > INT32_MAX) return QVIT_EINVAL;
  return QVIT_OK;
}

inline dim3 wave_grid(int64_t nitems) {
  const int64_t g = cdiv(nitems, kWaves);
  return dim3((unsigned)(g < 1 ? 1 : (g < kGridCap ? g : kGridCap)));
}

}  // namespace

#define QVIT_PRUNE_LAUNCH(KERNEL, GRID, ...)                                                               \
  do {                                                                                                     \
    if (variant == QVIT_QAT_SGD)                                                                           \
      hipLaunchKernelGGL(KERNEL<QVIT_QAT_SGD>, GRID, dim3(kThreads), 0, stream, __VA_ARGS__);              \
    else if (variant == QVIT_QAT_ADAM)                                                                     \
      hipLaunchKernelGGL(KERNEL<QVIT_QAT_ADAM>, GRID, dim3(kThreads), 0, stream, __VA_ARGS__);             \
    else                                                                                                   \
      hipLaunchKernelGGL(KERNEL<QVIT_QAT_ADAMW>, GRID, dim3(kThreads), 0, stream, __VA_ARGS__);            \
  } while (0)

extern "C" {

int qvit_prune_scores(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                      int64_t nitems, double* sums, int variant, int first_step, float lr, float lr_quant,
                      float first_momentum, float second_momentum, float alpha1, float alpha2, float weight_decay,
                      float bias_correction1, float bias_correction2, float clip_lo, float clip_hi,
                      hipStream_t stream) {
  if (const int st = tables_status(groups, ngroups, members, nmembers, items, nitems, sums)) return st;
  if (variant_status(variant)) return QVIT_EINVAL;
  if (ngroups == 0 || nmembers == 0 || nitems == 0) return QVIT_OK;
  const Hyper h = make_hyper(variant, first_step, lr, lr_quant, first_momentum, second_momentum, alpha1, alpha2,
                             weight_decay, bias_correction1, bias_correction2, clip_lo, clip_hi);
  QVIT_PRUNE_LAUNCH(prune_scores_kernel, wave_grid(nitems), static_cast<const PruneGroup*>(groups), ngroups,
                    static_cast<const PruneMember*>(members), nmembers, static_cast<const PruneItem*>(items), nitems,
                    sums, h);
  return qvit_launch_status();
}

int qvit_prune_scores_finish(const void* groups, int ngroups, const void* items, int64_t nitems, const double* sums,
                             double w_magnitude, double w_avg_magnitude, double w_cosine, double w_taylor1,
                             double w_taylor2, float* scores, hipStream_t stream) {
  if (!groups || !items || !sums || !scores) return QVIT_ENULL;
  if (qvit_misaligned(7, groups, items, sums) || qvit_misaligned(3, scores)) return QVIT_EALIGN;
  if (ngroups < 0 || nitems < 0 || nitems > INT32_MAX) return QVIT_EINVAL;
  if (ngroups == 0 || nitems == 0) return QVIT_OK;
  hipLaunchKernelGGL(prune_scores_finish_kernel, dim3(1), dim3(kThreads), 0, stream,
                     static_cast<const PruneGroup*>(groups), ngroups, static_cast<const PruneItem*>(items), nitems,
                     sums, w_magnitude, w_avg_magnitude, w_cosine, w_taylor1, w_taylor2, scores);
  return qvit_launch_status();
}

int qvit_prune_scores_fold(const void* groups, int ngroups, const void* items, int64_t nitems, const double* sums,
                           const void* units, int64_t nunits, double* unit_sums, hipStream_t stream) {
  if (!groups || !items || !sums || !units || !unit_sums) return QVIT_ENULL;
  if (qvit_misaligned(7, groups, items, sums, units, unit_sums)) return QVIT_EALIGN;
  if (ngroups < 0 || nitems < 0 || nitems > INT32_MAX || nunits < 0 || nunits > INT32_MAX) return QVIT_EINVAL;
  if (ngroups == 0 || nunits == 0) return QVIT_OK;
  hipLaunchKernelGGL(prune_scores_fold_kernel, dim3((unsigned)cdiv(nunits, kThreads)), dim3(kThreads), 0, stream,
                     static_cast<const PruneGroup*>(groups), ngroups, static_cast<const PruneItem*>(items), nitems,
                     sums, static_cast<const PruneItem*>(units), nunits, unit_sums);
  return qvit_launch_status();
}

int qvit_prune_joint_scalars(const void* quants, int nquants, int variant, int first_step, float lr, float lr_quant,
                             float first_momentum, float second_momentum, float alpha1, float alpha2,
                             float weight_decay, float bias_correction1, float bias_correction2, float clip_lo,
                             float clip_hi, int min_bit_act, int max_bit_act, hipStream_t stream) {
  if (!quants) return QVIT_ENULL;
  if (qvit_misaligned(7, quants)) return QVIT_EALIGN;
  if (nquants < 0) return QVIT_EINVAL;
  if (variant_status(variant)) return QVIT_EINVAL;
  if (min_bit_act < 2 || max_bit_act < min_bit_act || max_bit_act > 32) return QVIT_EINVAL;
  if (nquants == 0) return QVIT_OK;
  const Hyper h = make_hyper(variant, first_step, lr, lr_quant, first_momentum, second_momentum, alpha1, alpha2,
                             weight_decay, bias_correction1, bias_correction2, clip_lo, clip_hi);
  QVIT_PRUNE_LAUNCH(prune_joint_scalars_kernel, dim3((unsigned)cdiv(nquants, kThreads)),
                    static_cast<const QatQuant*>(quants), nquants, h, min_bit_act, max_bit_act);
  return qvit_launch_status();
}

int qvit_prune_joint_reduce(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                            int64_t nitems, double* partials, int variant, int first_step, float lr, float lr_quant,
                            float first_momentum, float second_momentum, float alpha1, float alpha2,
                            float weight_decay, float bias_correction1, float bias_correction2, float clip_lo,
                            float clip_hi, hipStream_t stream) {
  if (const int st = tables_status(groups, ngroups, members, nmembers, items, nitems, partials)) return st;
  if (variant_status(variant)) return QVIT_EINVAL;
  if (ngroups == 0 || nmembers == 0 || nitems == 0) return QVIT_OK;
  const Hyper h = make_hyper(variant, first_step, lr, lr_quant, first_momentum, second_momentum, alpha1, alpha2,
                             weight_decay, bias_correction1, bias_correction2, clip_lo, clip_hi);
  QVIT_PRUNE_LAUNCH(prune_joint_reduce_kernel, wave_grid(nitems), static_cast<const PruneGroup*>(groups), ngroups,
                    static_cast<const PruneMember*>(members), nmembers, static_cast<const PruneItem*>(items), nitems,
                    partials, h);
  return qvit_launch_status();
}

int qvit_prune_joint_finish(const void* groups, int ngroups, const double* partials, int64_t npartials, double lr,
                            int period, int t_in_period, int min_bit_wt, int max_bit_wt, float* gamma, int32_t* info,
                            hipStream_t stream) {
  if (!groups || !partials || !gamma || !info) return QVIT_ENULL;
  if (qvit_misaligned(7, groups, partials) || qvit_misaligned(3, gamma, info)) return QVIT_EALIGN;
  if (ngroups < 0 || npartials < 0 || npartials > INT32_MAX) return QVIT_EINVAL;
  if (period < 1 || t_in_period < 0 || t_in_period >= period) return QVIT_EINVAL;
  if (min_bit_wt < 2 || max_bit_wt < min_bit_wt || max_bit_wt > 32) return QVIT_EINVAL;
  if (ngroups == 0) return QVIT_OK;
  hipLaunchKernelGGL(prune_joint_finish_kernel, dim3((unsigned)ngroups), dim3(kThreads), 0, stream,
                     static_cast<const PruneGroup*>(groups), ngroups, partials, npartials, lr, period, t_in_period,
                     min_bit_wt, max_bit_wt, gamma, info);
  return qvit_launch_status();
}

int qvit_prune_joint_apply(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                           int64_t nitems, const float* gamma, int variant, int first_step, float lr, float lr_quant,
                           float first_momentum, float second_momentum, float alpha1, float alpha2,
                           float weight_decay, float bias_correction1, float bias_correction2, float clip_lo,
                           float clip_hi, hipStream_t stream) {
  if (const int st = tables_status(groups, ngroups, members, nmembers, items, nitems, gamma)) return st;
  if (variant_status(variant)) return QVIT_EINVAL;
  if (ngroups == 0 || nmembers == 0 || nitems == 0) return QVIT_OK;
  const Hyper h = make_hyper(variant, first_step, lr, lr_quant, first_momentum, second_momentum, alpha1, alpha2,
                             weight_decay, bias_correction1, bias_correction2, clip_lo, clip_hi);
  QVIT_PRUNE_LAUNCH(prune_joint_apply_kernel, wave_grid(nitems), static_cast<const PruneGroup*>(groups), ngroups,
                    static_cast<const PruneMember*>(members), nmembers, static_cast<const PruneItem*>(items), nitems,
                    gamma, h);
  return qvit_launch_status();
}

}  // extern "C"
