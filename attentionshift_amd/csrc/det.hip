// The box head's test-time stage before NMS for gfx950: what BBoxHead.get_bboxes and the front of multiclass_nms
// (mmdet/core/post_processing/bbox_nms.py:34-93) do to ONE image -- softmax, delta2bbox of all n x K boxes, rescale, threshold,
// three mask gathers, the class offsets, an argsort and a gather -- as select, order, decode only the survivors.
//
//   as_det_candidates   five launches, no host sync:
//     1. det_score_kernel    one wave per RoI row: the softmax of its K + 1 logits in registers (or the given scores), the
//                            probabilities stored, the row's number of scores above the threshold.
//     2. det_scan_kernel     one workgroup: the exclusive scan of the rows' counts; the total m -> cand_count.
//     3. det_keys_kernel     one wave per row: its candidates' 64-bit keys at the row's offset, columns ascending (ballots).
//     4. det_rank_kernel     one thread per candidate: its rank = the number of smaller keys, counted over LDS tiles of the key
//                            list (keys are distinct, m <= 65535); then the decode of that one box (delta2bbox, clip,
//                            rescale) written with its score, RoI and label at the rank.
//     5. det_finish_kernel   one workgroup: M = the largest coordinate, cand_nms_box = box + label * (M + 1) for as_nms.
//
// Key of candidate (r, c):  bits 63..32  ~u, u = the order-preserving unsigned image of the score (-0.0 folded onto +0.0; a NaN
//                                        is never a candidate)        bits 19..0  the flat index r * K + c  (n * K <= 2^20)
// Ascending key order is (score descending, flat index ascending): what a stable descending argsort of the compacted scores
// gives.  Every output position follows from the scan or the rank: no float atomics, nothing depends on thread timing.
//
// This file is compiled with -ffp-contract=off: apart from expf every step of the decode rounds like the ATen ops of
// bbox_loss.delta2bbox (separate multiply / add), and the divides (softmax, rescale) are correctly rounded.
#include "common.h"

namespace {

constexpr int DET_MAX_N = 65535;
constexpr int DET_MAX_K = 255;         // K + 1 <= 256 columns: four per lane
constexpr int DET_MAX_NK = 1 << 20;    // the flat index takes 20 bits of the key
constexpr int DET_CAP = 65535;         // as_nms' limit
constexpr int DET_COLS = 4;            // columns per lane of a row's wave
constexpr int DET_ROW_NT = 256;        // the row kernels: four rows (waves) per workgroup
constexpr int DET_ROWS = DET_ROW_NT / 64;
constexpr int DET_NT = 1024;           // the one-workgroup kernels (scan, finish)
constexpr int DET_WAVES = DET_NT / 64;
constexpr int DET_RANK_NT = 128;       // candidates per workgroup of the rank kernel
constexpr int DET_TILE = 1024;         // keys per LDS tile (8 KB)

struct DetParams {
  float mean[4], std[4], scale[4];
  float ih, iw, max_ratio;
  int clip, rescale;
};

// ascending in this = descending in the score (no NaN reaches it)
__device__ __forceinline__ unsigned det_desc_key(float v) {
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

// grid ceil(n / 4).  cnt[r] = the number of columns c < K of row r with p > thr; p -> probs (when not null)
__global__ __launch_bounds__(DET_ROW_NT) void det_score_kernel(const float* __restrict__ scores, int apply_softmax, int n, int K,
                                                               float thr, float* __restrict__ probs, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * DET_ROWS + (threadIdx.x >> 6);
  if (row >= n) return;
  const size_t o = (size_t)row * (K + 1);
  float p[DET_COLS];
#pragma unroll
  for (int j = 0; j < DET_COLS; ++j) {
    const int c = lane + 64 * j;
    p[j] = c <= K ? scores[o + c] : -INFINITY;
  }
  if (apply_softmax) {
    // a NaN or +inf logit makes every exp(x - max) of the row NaN or the sum NaN: NaN probabilities, as torch.softmax gives
    float mx = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3]));
    mx = wave_max(mx);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < DET_COLS; ++j) {
      p[j] = (lane + 64 * j) <= K ? expf(p[j] - mx) : 0.0f;
      s += p[j];
    }
    s = wave_sum(s);                                       // a butterfly: the same bits in every lane
#pragma unroll
    for (int j = 0; j < DET_COLS; ++j) p[j] = __fdiv_rn(p[j], s);
  }
  int c_row = 0;
#pragma unroll
  for (int j = 0; j < DET_COLS; ++j) {
    const int c = lane + 64 * j;
    if (probs && c <= K) probs[o + c] = p[j];
    c_row += __builtin_popcountll(__ballot(c < K && p[j] > thr));
  }
  if (lane == 0) cnt[row] = c_row;
}

// one workgroup: off[0..n) counts -> exclusive offsets in place, off[n] = cand_count[0] = the total
__global__ __launch_bounds__(DET_NT) void det_scan_kernel(int n, int* __restrict__ off, int* __restrict__ cand_count) {
  __shared__ int wsum[DET_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n + DET_NT - 1) / DET_NT;               // <= 64 consecutive rows per thread
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int mine = 0;
  for (int r = lo; r < hi; ++r) mine += off[r];
  const int incl_w = wave_incl_scan(mine, lane);
  if (lane == 63) wsum[wave] = incl_w;
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < DET_WAVES; ++w) {
    if (w < wave) before += wsum[w];
    total += wsum[w];
  }
  int run = before + incl_w - mine;
  for (int r = lo; r < hi; ++r) {
    const int c = off[r];
    off[r] = run;
    run += c;
  }
  if (tid == 0) {
    off[n] = total;
    cand_count[0] = total;
  }
}

// grid ceil(n / 4).  P = the scores the threshold applies to ([n, K+1]); keys[off[r] ..) = the keys of row r, columns ascending
__global__ __launch_bounds__(DET_ROW_NT) void det_keys_kernel(const float* __restrict__ P, int n, int K, float thr, int cap,
                                                              const int* __restrict__ off, unsigned long long* __restrict__ keys) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * DET_ROWS + (threadIdx.x >> 6);
  if (row >= n) return;
  const size_t o = (size_t)row * (K + 1);
  int pos = off[row];
#pragma unroll
  for (int j = 0; j < DET_COLS; ++j) {
    const int c = lane + 64 * j;
    const float p = c < K ? P[o + c] : 0.0f;
    const bool ok = c < K && p > thr;
    const unsigned long long bal = __ballot(ok);
    const int q = pos + __builtin_popcountll(bal & ((1ull << lane) - 1));
    if (ok && q < cap) keys[q] = ((unsigned long long)det_desc_key(p) << 32) | (unsigned)(row * K + c);
    pos += __builtin_popcountll(bal);
  }
}

// grid ceil(cap / DET_RANK_NT); workgroups past the count m leave at once, all of them when m > cap
__global__ __launch_bounds__(DET_RANK_NT) void det_rank_kernel(const unsigned long long* __restrict__ keys,
                                                               const int* __restrict__ cand_count, int cap,
                                                               const float* __restrict__ P, const float* __restrict__ rois,
                                                               const float* __restrict__ deltas, int K, int Kb, DetParams pr,
                                                               float4* __restrict__ cand_box, float* __restrict__ cand_score,
                                                               int* __restrict__ cand_roi, int* __restrict__ cand_label) {
  __shared__ unsigned long long tile[DET_TILE];
  const int m = cand_count[0], tid = threadIdx.x;
  if (m > cap || (int)(blockIdx.x * DET_RANK_NT) >= m) return;      // uniform over the workgroup
  const int i = blockIdx.x * DET_RANK_NT + tid;
  const unsigned long long key = i < m ? keys[i] : ~0ull;
  int rank = 0;
  for (int t0 = 0; t0 < m; t0 += DET_TILE) {
    __syncthreads();
    for (int j = tid; j < DET_TILE; j += DET_RANK_NT) tile[j] = t0 + j < m ? keys[t0 + j] : ~0ull;   // the padding is below no key
    __syncthreads();
    const int lim = min(DET_TILE, (m - t0 + 7) & ~7);
    for (int j = 0; j < lim; j += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) rank += tile[j + u] < key ? 1 : 0;   // one address per wave: a broadcast read
    }
  }
  if (i >= m || rank >= m) return;                         // (distinct keys: rank < m always)
  const int flat = (int)(key & (unsigned)(DET_MAX_NK - 1)), r = flat / K, c = flat - r * K, cb = Kb == 1 ? 0 : c;
  float4 box;
  if (deltas) {
    const float4 roi = *reinterpret_cast<const float4*>(rois + (size_t)4 * r);
    const float* dp = deltas + ((size_t)r * Kb + cb) * 4;
    const float d0 = dp[0] * pr.std[0] + pr.mean[0];
    const float d1 = dp[1] * pr.std[1] + pr.mean[1];
    float d2 = dp[2] * pr.std[2] + pr.mean[2];
    float d3 = dp[3] * pr.std[3] + pr.mean[3];
    d2 = nan_min(nan_max(d2, -pr.max_ratio), pr.max_ratio);
    d3 = nan_min(nan_max(d3, -pr.max_ratio), pr.max_ratio);
    const float px = (roi.x + roi.z) * 0.5f, py = (roi.y + roi.w) * 0.5f, pw = roi.z - roi.x, ph = roi.w - roi.y;
    const float gw = pw * expf(d2), gh = ph * expf(d3);
    const float gx = px + pw * d0, gy = py + ph * d1;
    box.x = gx - gw * 0.5f;
    box.y = gy - gh * 0.5f;
    box.z = gx + gw * 0.5f;
    box.w = gy + gh * 0.5f;
    if (pr.clip) {
      box.x = nan_min(nan_max(box.x, 0.0f), pr.iw);
      box.y = nan_min(nan_max(box.y, 0.0f), pr.ih);
      box.z = nan_min(nan_max(box.z, 0.0f), pr.iw);
      box.w = nan_min(nan_max(box.w, 0.0f), pr.ih);
    }
  } else {
    box = *reinterpret_cast<const float4*>(rois + ((size_t)r * Kb + cb) * 4);
  }
  if (pr.rescale) {
    box.x = __fdiv_rn(box.x, pr.scale[0]);
    box.y = __fdiv_rn(box.y, pr.scale[1]);
    box.z = __fdiv_rn(box.z, pr.scale[2]);
    box.w = __fdiv_rn(box.w, pr.scale[3]);
  }
  cand_box[rank] = box;
  cand_score[rank] = P[(size_t)r * (K + 1) + c];
  cand_roi[rank] = r;
  cand_label[rank] = c;
}

// one workgroup
__global__ __launch_bounds__(DET_NT) void det_finish_kernel(const int* __restrict__ cand_count, int cap,
                                                            const float4* __restrict__ cand_box, const int* __restrict__ cand_label,
                                                            float4* __restrict__ cand_nms_box) {
  __shared__ float wmax[DET_WAVES];
  const int m = cand_count[0], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (m > cap) return;
  // M, NaN propagating like Tensor.max()
  float mx = -INFINITY;
  for (int j = tid; j < m; j += DET_NT) {
    const float4 b = cand_box[j];
    mx = nan_max(mx, nan_max(nan_max(b.x, b.y), nan_max(b.z, b.w)));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = nan_max(mx, __shfl_xor(mx, s));
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  float M = wmax[0];
  for (int w = 1; w < DET_WAVES; ++w) M = nan_max(M, wmax[w]);
  const float step = M + 1.0f;
  for (int j = tid; j < m; j += DET_NT) {
    const float4 b = cand_box[j];
    const float o = (float)cand_label[j] * step;
    cand_nms_box[j] = make_float4(b.x + o, b.y + o, b.z + o, b.w + o);
  }
}

inline size_t det_round16(size_t b) { return (b + 15) & ~(size_t)15; }
inline int det_cap(int n, int K) { return (long long)n * K < DET_CAP ? n * K : DET_CAP; }

}  // namespace

extern "C" size_t as_det_candidates_workspace_bytes(int n, int K) {
  if (n <= 0 || K <= 0) return 0;
  const size_t cap = (size_t)n * K < (size_t)DET_CAP ? (size_t)n * K : (size_t)DET_CAP;
  return det_round16(8 * cap) + det_round16(4 * ((size_t)n + 1)) + det_round16(4 * (size_t)n * ((size_t)K + 1));
}

extern "C" int as_det_candidates(const float* rois_or_boxes, const float* deltas, int Kb, const float* scores, int apply_softmax,
                                 int n, int K, float score_thr, const float* img_shape, const float* scale,
                                 const float* means_stds, float max_ratio, float* prob_out, float* cand_box, float* cand_nms_box,
                                 float* cand_score, int32_t* cand_roi, int32_t* cand_label, int32_t* cand_count, void* workspace,
                                 size_t workspace_bytes, as_stream_t stream) {
  AS_REQUIRE(n >= 0 && K >= 1, AS_E_BADARG, "as_det_candidates: n = %d, K = %d", n, K);
  AS_REQUIRE(Kb == 1 || Kb == K, AS_E_BADARG, "as_det_candidates: Kb = %d is neither 1 nor K = %d", Kb, K);
  AS_REQUIRE(!deltas || means_stds, AS_E_BADARG, "as_det_candidates: null means_stds with deltas");
  AS_REQUIRE(n <= DET_MAX_N && K <= DET_MAX_K && (long long)n * K <= DET_MAX_NK, AS_E_UNSUPPORTED,
             "as_det_candidates: n = %d > %d, K = %d > %d or n * K > 2^20", n, DET_MAX_N, K, DET_MAX_K);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (cand_count) {
      const hipError_t e = hipMemsetAsync(cand_count, 0, sizeof(int32_t), s);
      AS_REQUIRE(e == hipSuccess, AS_E_LAUNCH, "as_det_candidates: memset failed: %s", hipGetErrorString(e));
    }
    return AS_OK;
  }
  AS_REQUIRE(rois_or_boxes && scores && cand_box && cand_nms_box && cand_score && cand_roi && cand_label && cand_count &&
                 workspace,
             AS_E_BADARG, "as_det_candidates: null pointer");
  const size_t need = as_det_candidates_workspace_bytes(n, K);
  AS_REQUIRE(workspace_bytes >= need, AS_E_WORKSPACE, "as_det_candidates: workspace of %zu bytes, %zu needed", workspace_bytes,
             need);
  AS_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(cand_box) |
               reinterpret_cast<uintptr_t>(cand_nms_box) | reinterpret_cast<uintptr_t>(rois_or_boxes)) & 15) == 0,
             AS_E_BADARG, "as_det_candidates: workspace / cand_box / cand_nms_box / rois_or_boxes not 16-byte aligned");
  const int cap = det_cap(n, K);
  char* w = static_cast<char*>(workspace);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(w);
  int* off = reinterpret_cast<int*>(w + det_round16(8 * (size_t)cap));
  float* ws_prob = reinterpret_cast<float*>(w + det_round16(8 * (size_t)cap) + det_round16(4 * ((size_t)n + 1)));
  // the scores the threshold applies to: given ones are read where they are, a softmax lands in prob_out or the workspace
  float* probs = apply_softmax ? (prob_out ? prob_out : ws_prob) : prob_out;
  const float* P = apply_softmax ? probs : scores;
  DetParams pr;
  memset(&pr, 0, sizeof(pr));
  for (int c = 0; c < 4; ++c) {
    pr.mean[c] = means_stds ? means_stds[c] : 0.0f;
    pr.std[c] = means_stds ? means_stds[4 + c] : 1.0f;
    pr.scale[c] = scale ? scale[c] : 1.0f;
  }
  pr.clip = img_shape != nullptr;
  pr.ih = img_shape ? img_shape[0] : 0.0f;
  pr.iw = img_shape ? img_shape[1] : 0.0f;
  pr.rescale = scale != nullptr;
  pr.max_ratio = max_ratio;
  const int row_grid = as_ceil_div(n, DET_ROWS);
  hipLaunchKernelGGL(det_score_kernel, dim3(row_grid), dim3(DET_ROW_NT), 0, s, scores, apply_softmax, n, K, score_thr, probs, off);
  hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(DET_NT), 0, s, n, off, cand_count);
  hipLaunchKernelGGL(det_keys_kernel, dim3(row_grid), dim3(DET_ROW_NT), 0, s, P, n, K, score_thr, cap, off, keys);
  hipLaunchKernelGGL(det_rank_kernel, dim3(as_ceil_div(cap, DET_RANK_NT)), dim3(DET_RANK_NT), 0, s, keys, cand_count, cap, P,
                     rois_or_boxes, deltas, K, Kb, pr, reinterpret_cast<float4*>(cand_box), cand_score, cand_roi, cand_label);
  hipLaunchKernelGGL(det_finish_kernel, dim3(1), dim3(DET_NT), 0, s, cand_count, cap, reinterpret_cast<const float4*>(cand_box),
                     cand_label, reinterpret_cast<float4*>(cand_nms_box));
  AS_CHECK_LAUNCH("det_candidates");
  return AS_OK;
}
