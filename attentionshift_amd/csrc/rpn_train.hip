// RPN training targets for gfx950: what mmdet/models/dense_heads/anchor_head.py:175-271 (_get_targets_single) does for every
// image -- valid / inside flags, MaxIoUAssigner, the index side of RandomSampler, bbox2delta -- without an anchor tensor, an
// IoU matrix or a dense target tensor.
//
//   as_rpn_assign    a memset and three launches for all B images and L levels:
//     1. rpn_iou_kernel    one thread per (image, anchor), the image's boxes in LDS: the inside flag, the largest IoU and its
//                          lowest box index; per box the largest IoU over the inside anchors, reduced in LDS and combined
//                          across workgroups by an unsigned integer max on the IoU's bits (IoUs are >= 0, so the order of the
//                          bits is the order of the values and the result does not depend on arrival order).
//     2. rpn_rule_kernel   the assignment rule; the low-quality match recomputes the IoU with box g by the same instructions
//                          (the same bits, so == is exact).  Every workgroup leaves its number of positives and negatives.
//     3. rpn_scan_kernel   one workgroup per image: the exclusive scan of those per-workgroup counts and the image's totals.
//   as_rpn_sample    one workgroup per (image, set): the r-th positive / negative in anchor order from the scanned counts (a
//                    binary search for the 256-anchor block, four ballots inside it), then a bitonic sort of the indices.
//   as_rpn_targets   one thread per sampled positive: its box index and bbox2delta of the anchor computed from (level, index).
//
// Anchor t of an image is level l, i = (y * W_l + x) * A + a, t = offset_l + i (the order of as_rpn_candidates).
//
// This file is compiled with -ffp-contract=off: every step of the IoU is one correctly rounded fp32 operation in the order
// of assign.bbox_overlaps, and apart from logf every step of the targets rounds like the ATen ops of bbox_loss.bbox2delta.
// There is no float atomic anywhere: every output is bitwise reproducible.
#include <limits.h>

#include "common.h"

namespace {

constexpr int RT_NT = 256;             // anchors per workgroup of the iou / rule kernels = the block of the rank search
constexpr int RT_MAX_L = 8;
constexpr int RT_MAX_G = 1024;         // boxes of one image: 16 KB of coordinates + 4 KB of areas + 4 KB of maxima in LDS
constexpr int RT_MAX_NUM = 2048;       // sampled anchors per (image, set): one bitonic sort of 8 KB in LDS
constexpr int RT_SNT = 1024;           // threads of the scan and sample kernels
constexpr int RT_SWAVES = RT_SNT / 64;
constexpr int RT_IDX_BITS = 28;

struct RtLevels {
  int H[RT_MAX_L], W[RT_MAX_L], sx[RT_MAX_L], sy[RT_MAX_L];
  int off[RT_MAX_L + 1];               // first anchor of the level; off[L] = T
};
struct RtRule {
  float pos_thr, neg_thr, min_pos;
  int match_low_quality, allowed_border;
};
struct RtNorm {
  float mean[4], std[4];
};

// anchor t -> (level, x, y, a) and its coordinates
__device__ __forceinline__ void anchor_of(const RtLevels& lv, int L, int A, int t, const float* __restrict__ base_anchors, int* l_out,
                                          int* x_out, int* y_out, float* a4) {
  int l = 0;
  for (int k = 1; k < L; ++k)
    if (t >= lv.off[k]) l = k;
  const int i = t - lv.off[l];
  const int p = i / A, a = i - p * A, W = lv.W[l];
  const int y = p / W, x = p - y * W;
  const float* ba = base_anchors + ((size_t)l * A + a) * 4;
  const float shx = (float)(x * lv.sx[l]), shy = (float)(y * lv.sy[l]);
  a4[0] = ba[0] + shx; a4[1] = ba[1] + shy; a4[2] = ba[2] + shx; a4[3] = ba[3] + shy;
  *l_out = l; *x_out = x; *y_out = y;
}

// AnchorGenerator.valid_flags + anchor_inside_flags; shp = (pad_h, pad_w, img_h, img_w)
__device__ __forceinline__ bool anchor_inside(const RtLevels& lv, int l, int x, int y, const float* a4, const int* __restrict__ shp,
                                              int border) {
  const int sx = lv.sx[l] > 0 ? lv.sx[l] : 1, sy = lv.sy[l] > 0 ? lv.sy[l] : 1;
  const int vh = min((shp[0] + sy - 1) / sy, lv.H[l]), vw = min((shp[1] + sx - 1) / sx, lv.W[l]);
  bool in = x < vw && y < vh;
  if (border >= 0) {
    const float lo = (float)(-border), hx = (float)(shp[3] + border), hy = (float)(shp[2] + border);
    in = in && a4[0] >= lo && a4[1] >= lo && a4[2] < hx && a4[3] < hy;
  }
  return in;
}

// assign.bbox_overlaps(gt, anchor, eps = 1e-6), operation by operation
__device__ __forceinline__ float iou_of(float gx1, float gy1, float gx2, float gy2, float garea, const float* a4, float aarea) {
  const float w = fmaxf(fminf(gx2, a4[2]) - fmaxf(gx1, a4[0]), 0.0f);
  const float h = fmaxf(fminf(gy2, a4[3]) - fmaxf(gy1, a4[1]), 0.0f);
  const float inter = w * h;
  const float uni = (garea + aarea) - inter;
  return __fdiv_rn(inter, fmaxf(uni, 1e-6f));
}

__device__ __forceinline__ void load_boxes(const float* __restrict__ gt, int g0, int G, float4* sbox, float* sarea, int tid, int nt) {
  for (int g = tid; g < G; g += nt) {
    const float* p = gt + (size_t)(g0 + g) * 4;
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    sbox[g] = make_float4(x1, y1, x2, y2);
    sarea[g] = (x2 - x1) * (y2 - y1);
  }
}

// grid (ceil(T / RT_NT), B).  assigned <- -2 outside, else the lowest argmax (rewritten by rpn_rule_kernel)
__global__ __launch_bounds__(RT_NT) void rpn_iou_kernel(RtLevels lv, int L, int A, int T, const float* __restrict__ base_anchors,
                                                        const float* __restrict__ gt, const int* __restrict__ gt_off, int sum_g,
                                                        const int* __restrict__ shapes, int border, int* __restrict__ assigned,
                                                        float* __restrict__ max_iou, unsigned* __restrict__ gt_max) {
  __shared__ float4 sbox[RT_MAX_G];
  __shared__ float sarea[RT_MAX_G];
  __shared__ unsigned smax[RT_MAX_G];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int g0 = max(min(gt_off[b], sum_g), 0);
  const int G = max(min(min(gt_off[b + 1], sum_g) - g0, RT_MAX_G), 0);
  load_boxes(gt, g0, G, sbox, sarea, tid, RT_NT);
  for (int g = tid; g < G; g += RT_NT) smax[g] = 0u;
  __syncthreads();
  const int t = blockIdx.x * RT_NT + tid;
  if (t < T) {
    int l, x, y;
    float a4[4];
    anchor_of(lv, L, A, t, base_anchors, &l, &x, &y, a4);
    const size_t o = (size_t)b * T + t;
    if (!anchor_inside(lv, l, x, y, a4, shapes + 4 * b, border)) {
      assigned[o] = -2;
      max_iou[o] = 0.0f;
    } else {
      const float aarea = (a4[2] - a4[0]) * (a4[3] - a4[1]);
      float best = -INFINITY;
      int arg = 0;
      for (int g = 0; g < G; ++g) {
        const float4 bx = sbox[g];
        const float iou = iou_of(bx.x, bx.y, bx.z, bx.w, sarea[g], a4, aarea);
        if (iou > best) {
          best = iou;
          arg = g;
        }
        if (iou > 0.0f) atomicMax(&smax[g], __float_as_uint(iou));
      }
      assigned[o] = arg;
      max_iou[o] = G > 0 ? best : 0.0f;
    }
  }
  __syncthreads();
  for (int g = tid; g < G; g += RT_NT)
    if (smax[g] != 0u) atomicMax(&gt_max[g0 + g], smax[g]);
}

// grid (ceil(T / RT_NT), B).  blk_cnt [B, nblk, 2] <- (positives, negatives) of every workgroup
__global__ __launch_bounds__(RT_NT) void rpn_rule_kernel(RtLevels lv, int L, int A, int T, const float* __restrict__ base_anchors,
                                                         const float* __restrict__ gt, const int* __restrict__ gt_off, int sum_g, RtRule rule,
                                                         int* __restrict__ assigned, const float* __restrict__ max_iou,
                                                         const unsigned* __restrict__ gt_max, int* __restrict__ blk_cnt) {
  __shared__ float4 sbox[RT_MAX_G];
  __shared__ float sarea[RT_MAX_G];
  __shared__ float sgmax[RT_MAX_G];
  __shared__ int wcnt[2][RT_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  const int g0 = max(min(gt_off[b], sum_g), 0);
  const int G = max(min(min(gt_off[b + 1], sum_g) - g0, RT_MAX_G), 0);
  const bool mlq = rule.match_low_quality != 0 && G > 0;
  if (mlq) {
    load_boxes(gt, g0, G, sbox, sarea, tid, RT_NT);
    for (int g = tid; g < G; g += RT_NT) sgmax[g] = __uint_as_float(gt_max[g0 + g]);
  }
  __syncthreads();
  const int t = blockIdx.x * RT_NT + tid;
  int res = -2;
  if (t < T) {
    const size_t o = (size_t)b * T + t;
    const int arg = assigned[o];
    if (arg != -2) {
      if (G == 0) {
        res = 0;
      } else {
        const float m = max_iou[o];
        res = -1;
        if (m >= 0.0f && m < rule.neg_thr) res = 0;
        if (m >= rule.pos_thr) res = arg + 1;
        if (mlq) {
          int l, x, y;
          float a4[4];
          anchor_of(lv, L, A, t, base_anchors, &l, &x, &y, a4);
          const float aarea = (a4[2] - a4[0]) * (a4[3] - a4[1]);
          for (int g = 0; g < G; ++g) {
            const float gm = sgmax[g];
            if (gm >= rule.min_pos) {
              const float4 bx = sbox[g];
              if (iou_of(bx.x, bx.y, bx.z, bx.w, sarea[g], a4, aarea) == gm) res = g + 1;
            }
          }
        }
      }
      assigned[o] = res;
    }
  }
  const unsigned long long bp = __ballot(res > 0), bn = __ballot(res == 0);
  if (lane == 0) {
    wcnt[0][wave] = __builtin_popcountll(bp);
    wcnt[1][wave] = __builtin_popcountll(bn);
  }
  __syncthreads();
  if (tid < 2) {
    int s = 0;
    for (int w = 0; w < RT_NT / 64; ++w) s += wcnt[tid][w];
    blk_cnt[((size_t)b * gridDim.x + blockIdx.x) * 2 + tid] = s;
  }
}

// one workgroup per image: blk_cnt -> its exclusive scan (in place), counts [B,2] <- the totals
__global__ __launch_bounds__(RT_SNT) void rpn_scan_kernel(int nblk, int* __restrict__ blk_cnt, int* __restrict__ counts) {
  __shared__ int wsum[2][2][RT_SWAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  int* c = blk_cnt + (size_t)b * nblk * 2;
  int carry0 = 0, carry1 = 0, parity = 0;
  for (int base = 0; base < nblk; base += RT_SNT) {
    const int j = base + tid;
    const int v0 = j < nblk ? c[2 * j] : 0, v1 = j < nblk ? c[2 * j + 1] : 0;
    const int i0 = wave_incl_scan(v0, lane), i1 = wave_incl_scan(v1, lane);
    if (lane == 63) {
      wsum[parity][0][wave] = i0;
      wsum[parity][1][wave] = i1;
    }
    __syncthreads();
    int b0 = 0, b1 = 0, t0 = 0, t1 = 0;
    for (int w = 0; w < RT_SWAVES; ++w) {
      const int s0 = wsum[parity][0][w], s1 = wsum[parity][1][w];
      if (w < wave) {
        b0 += s0;
        b1 += s1;
      }
      t0 += s0;
      t1 += s1;
    }
    if (j < nblk) {
      c[2 * j] = carry0 + b0 + i0 - v0;
      c[2 * j + 1] = carry1 + b1 + i1 - v1;
    }
    carry0 += t0;
    carry1 += t1;
    parity ^= 1;
  }
  if (tid == 0) {
    counts[2 * b] = carry0;
    counts[2 * b + 1] = carry1;
  }
}

// grid (2, B): set 0 = positives (assigned > 0), set 1 = negatives (assigned == 0).  plan [B,4] = (n_pos, all_pos, n_neg,
// all_neg): n sampled anchors, the ranks 0 .. n-1 when `all`, else ranks [B,2,num].  out [B,2,num]: ascending, -1 past n.
__global__ __launch_bounds__(RT_SNT) void rpn_sample_kernel(int T, int nblk, int num, const int* __restrict__ assigned,
                                                            const int* __restrict__ blk_scan, const int* __restrict__ plan,
                                                            const int* __restrict__ ranks, int* __restrict__ out) {
  __shared__ int buf[RT_MAX_NUM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, set = blockIdx.x, b = blockIdx.y;
  const int n = max(min(plan[4 * b + 2 * set], num), 0);
  const bool all = plan[4 * b + 2 * set + 1] != 0;
  int P = 2;
  while (P < n) P <<= 1;
  for (int j = tid; j < P; j += RT_SNT) buf[j] = INT_MAX;
  __syncthreads();
  const int* scan = blk_scan + (size_t)b * nblk * 2 + set;
  const int* asg = assigned + (size_t)b * T;
  const int* rk = ranks + ((size_t)b * 2 + set) * num;
  for (int j = wave; j < n; j += RT_SWAVES) {              // one wave per sampled anchor
    const int r = all ? j : rk[j];
    if (r < 0) continue;
    int lo = 0, hi = nblk - 1;                             // the last block whose scanned count is <= r
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (scan[2 * mid] <= r) lo = mid; else hi = mid - 1;
    }
    int rem = r - scan[2 * lo];
    for (int c = 0; c < RT_NT / 64; ++c) {
      const int t = lo * RT_NT + c * 64 + lane;
      const int v = t < T ? asg[t] : -2;
      const bool hit = set == 0 ? v > 0 : v == 0;
      const unsigned long long bal = __ballot(hit);
      const int cnt = __builtin_popcountll(bal);
      if (rem < cnt) {
        if (hit && __builtin_popcountll(bal & ((1ull << lane) - 1)) == rem) buf[j] = t;
        break;
      }
      rem -= cnt;
    }
  }
  __syncthreads();
  bitonic_sort<int, RT_SNT>(buf, P, tid);
  int* o = out + ((size_t)b * 2 + set) * num;
  for (int j = tid; j < num; j += RT_SNT) {
    const int v = j < n ? buf[j] : INT_MAX;
    o[j] = v == INT_MAX ? -1 : v;
  }
}

// grid (ceil(num / RT_NT), B): pos_inds [B, stride] (the first num of every row)
__global__ __launch_bounds__(RT_NT) void rpn_targets_kernel(RtLevels lv, int L, int A, int T, const float* __restrict__ base_anchors,
                                                            const float* __restrict__ gt, const int* __restrict__ gt_off, int sum_g,
                                                            const int* __restrict__ assigned, const int* __restrict__ pos_inds,
                                                            int stride, int num, RtNorm nm, int* __restrict__ pos_gt,
                                                            float* __restrict__ pos_delta) {
  const int j = blockIdx.x * RT_NT + threadIdx.x, b = blockIdx.y;
  if (j >= num) return;
  const int t = pos_inds[(size_t)b * stride + j];
  const size_t o = (size_t)b * num + j;
  int g = -1;
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int g0 = max(min(gt_off[b], sum_g), 0), G = min(gt_off[b + 1], sum_g) - g0;
  if (t >= 0 && t < T) {
    g = assigned[(size_t)b * T + t] - 1;
    if (g >= 0 && g < G) {
      int l, x, y;
      float a4[4];
      anchor_of(lv, L, A, t, base_anchors, &l, &x, &y, a4);
      const float* p = gt + (size_t)(g0 + g) * 4;
      const float px = (a4[0] + a4[2]) * 0.5f, py = (a4[1] + a4[3]) * 0.5f, pw = a4[2] - a4[0], ph = a4[3] - a4[1];
      const float gx = (p[0] + p[2]) * 0.5f, gy = (p[1] + p[3]) * 0.5f, gw = p[2] - p[0], gh = p[3] - p[1];
      d[0] = __fdiv_rn(gx - px, pw);
      d[1] = __fdiv_rn(gy - py, ph);
      d[2] = logf(__fdiv_rn(gw, pw));
      d[3] = logf(__fdiv_rn(gh, ph));
#pragma unroll
      for (int c = 0; c < 4; ++c) d[c] = __fdiv_rn(d[c] - nm.mean[c], nm.std[c]);
    } else {
      g = -1;
    }
  }
  pos_gt[o] = g;
  *reinterpret_cast<float4*>(pos_delta + 4 * o) = make_float4(d[0], d[1], d[2], d[3]);
}

// -> T, -1 when a level is malformed, -2 when beyond the limits
long long rt_plan(const as_rpn_level* levels, int L, int A, RtLevels* lv) {
  long long T = 0;
  bool too_big = false;
  for (int l = 0; l < L; ++l) {
    if (levels[l].H <= 0 || levels[l].W <= 0 || levels[l].stride_x <= 0 || levels[l].stride_y <= 0) return -1;
    if ((long long)levels[l].stride_x * levels[l].W >= (1 << 24) || (long long)levels[l].stride_y * levels[l].H >= (1 << 24)) return -1;
    const long long n = (long long)A * levels[l].H * levels[l].W;
    if (n >= (1ll << RT_IDX_BITS)) too_big = true;
    lv->H[l] = levels[l].H; lv->W[l] = levels[l].W;
    lv->sx[l] = levels[l].stride_x; lv->sy[l] = levels[l].stride_y;
    lv->off[l] = (int)(too_big ? 0 : T);
    T += n;
  }
  if (too_big) return -2;
  lv->off[L] = (int)T;
  return T;
}

size_t rt_gt_bytes(int sumG) { return (size_t)16 * (size_t)((sumG + 3) / 4); }

}  // namespace

extern "C" size_t as_rpn_assign_workspace_bytes(int B, int T, int sumG) {
  if (B <= 0 || T <= 0 || sumG < 0) return 0;
  return rt_gt_bytes(sumG) + (size_t)8 * (size_t)B * (size_t)as_ceil_div(T, RT_NT);
}

#define RT_LEVEL_CHECKS(fn)                                                                                                        \
  AS_REQUIRE(levels, AS_E_BADARG, fn ": null host pointer");                                                                       \
  AS_REQUIRE(L >= 1 && L <= RT_MAX_L, AS_E_BADARG, fn ": L = %d outside 1 .. %d", L, RT_MAX_L);                                   \
  AS_REQUIRE(A >= 1 && B >= 0, AS_E_BADARG, fn ": A = %d, B = %d", A, B);                                                          \
  RtLevels lv;                                                                                                                     \
  memset(&lv, 0, sizeof(lv));                                                                                                      \
  const long long Tx = rt_plan(levels, L, A, &lv);                                                                                 \
  AS_REQUIRE(Tx != -1, AS_E_BADARG, fn ": a level with H, W or a stride <= 0, or shifts not exact in fp32");                       \
  AS_REQUIRE(Tx != -2, AS_E_UNSUPPORTED, fn ": a level of 2^%d anchors or more", RT_IDX_BITS);                                    \
  AS_REQUIRE(B <= 65535, AS_E_UNSUPPORTED, fn ": B = %d > 65535", B);                                                              \
  const int T = (int)Tx

extern "C" int as_rpn_assign(const as_rpn_level* levels, int L, int B, int A, const float* base_anchors, const float* gt_boxes,
                             const int32_t* gt_offsets, int sum_g, int max_g, const int32_t* shapes, float pos_iou_thr,
                             float neg_iou_thr, float min_pos_iou, int match_low_quality, int allowed_border, int32_t* assigned,
                             float* max_iou, int32_t* counts, void* workspace, size_t workspace_bytes, as_stream_t stream) {
  RT_LEVEL_CHECKS("as_rpn_assign");
  AS_REQUIRE(sum_g >= 0 && max_g >= 0 && max_g <= sum_g, AS_E_BADARG, "as_rpn_assign: sum_g = %d, max_g = %d", sum_g, max_g);
  AS_REQUIRE(max_g <= RT_MAX_G, AS_E_UNSUPPORTED, "as_rpn_assign: %d boxes in an image, at most %d", max_g, RT_MAX_G);
  if (B == 0) return AS_OK;
  AS_REQUIRE(base_anchors && gt_offsets && shapes && assigned && max_iou && counts && workspace && (gt_boxes || sum_g == 0),
             AS_E_BADARG, "as_rpn_assign: null pointer");
  const size_t need = as_rpn_assign_workspace_bytes(B, T, sum_g);
  AS_REQUIRE(workspace_bytes >= need, AS_E_WORKSPACE, "as_rpn_assign: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  AS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, AS_E_BADARG, "as_rpn_assign: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* w = static_cast<char*>(workspace);
  unsigned* gt_max = reinterpret_cast<unsigned*>(w);
  int* blk = reinterpret_cast<int*>(w + rt_gt_bytes(sum_g));
  const int nblk = as_ceil_div(T, RT_NT);
  if (sum_g > 0 && hipMemsetAsync(gt_max, 0, rt_gt_bytes(sum_g), s) != hipSuccess) {
    as_set_error("as_rpn_assign: memset failed");
    return AS_E_LAUNCH;
  }
  RtRule rule;
  rule.pos_thr = pos_iou_thr; rule.neg_thr = neg_iou_thr; rule.min_pos = min_pos_iou;
  rule.match_low_quality = match_low_quality; rule.allowed_border = allowed_border;
  hipLaunchKernelGGL(rpn_iou_kernel, dim3(nblk, B), dim3(RT_NT), 0, s, lv, L, A, T, base_anchors, gt_boxes, gt_offsets, sum_g, shapes,
                     allowed_border, assigned, max_iou, gt_max);
  hipLaunchKernelGGL(rpn_rule_kernel, dim3(nblk, B), dim3(RT_NT), 0, s, lv, L, A, T, base_anchors, gt_boxes, gt_offsets, sum_g, rule, assigned,
                     max_iou, gt_max, blk);
  hipLaunchKernelGGL(rpn_scan_kernel, dim3(B), dim3(RT_SNT), 0, s, nblk, blk, counts);
  AS_CHECK_LAUNCH("rpn_assign");
  return AS_OK;
}

extern "C" int as_rpn_sample(int B, int T, int sum_g, int num, const int32_t* assigned, const int32_t* plan, const int32_t* ranks,
                             const void* workspace, size_t workspace_bytes, int32_t* inds, as_stream_t stream) {
  AS_REQUIRE(B >= 0 && T >= 1 && sum_g >= 0 && num >= 1, AS_E_BADARG, "as_rpn_sample: B = %d, T = %d, sum_g = %d, num = %d", B, T,
             sum_g, num);
  AS_REQUIRE(num <= RT_MAX_NUM, AS_E_UNSUPPORTED, "as_rpn_sample: num = %d > %d", num, RT_MAX_NUM);
  AS_REQUIRE(B <= 65535, AS_E_UNSUPPORTED, "as_rpn_sample: B = %d > 65535", B);
  if (B == 0) return AS_OK;
  AS_REQUIRE(assigned && plan && ranks && workspace && inds, AS_E_BADARG, "as_rpn_sample: null pointer");
  const size_t need = as_rpn_assign_workspace_bytes(B, T, sum_g);
  AS_REQUIRE(workspace_bytes >= need, AS_E_WORKSPACE, "as_rpn_sample: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int* blk = reinterpret_cast<const int*>(static_cast<const char*>(workspace) + rt_gt_bytes(sum_g));
  hipLaunchKernelGGL(rpn_sample_kernel, dim3(2, B), dim3(RT_SNT), 0, (hipStream_t)stream, T, as_ceil_div(T, RT_NT), num, assigned, blk,
                     plan, ranks, inds);
  AS_CHECK_LAUNCH("rpn_sample");
  return AS_OK;
}

extern "C" int as_rpn_targets(const as_rpn_level* levels, int L, int B, int A, const float* base_anchors, const float* gt_boxes,
                              const int32_t* gt_offsets, int sum_g, const int32_t* assigned, const int32_t* pos_inds, int inds_stride,
                              int num,
                              const float* means_stds, int32_t* pos_gt, float* pos_delta, as_stream_t stream) {
  RT_LEVEL_CHECKS("as_rpn_targets");
  AS_REQUIRE(means_stds, AS_E_BADARG, "as_rpn_targets: null host pointer");
  AS_REQUIRE(num >= 1 && inds_stride >= num && sum_g >= 0, AS_E_BADARG, "as_rpn_targets: num = %d, inds_stride = %d, sum_g = %d", num,
             inds_stride, sum_g);
  AS_REQUIRE(num <= RT_MAX_NUM, AS_E_UNSUPPORTED, "as_rpn_targets: num = %d > %d", num, RT_MAX_NUM);
  if (B == 0) return AS_OK;
  AS_REQUIRE(base_anchors && gt_offsets && assigned && pos_inds && pos_gt && pos_delta && (gt_boxes || sum_g == 0), AS_E_BADARG,
             "as_rpn_targets: null pointer");
  AS_REQUIRE((reinterpret_cast<uintptr_t>(pos_delta) & 15) == 0, AS_E_BADARG, "as_rpn_targets: pos_delta not 16-byte aligned");
  RtNorm nm;
  for (int c = 0; c < 4; ++c) {
    nm.mean[c] = means_stds[c];
    nm.std[c] = means_stds[4 + c];
  }
  hipLaunchKernelGGL(rpn_targets_kernel, dim3(as_ceil_div(num, RT_NT), B), dim3(RT_NT), 0, (hipStream_t)stream, lv, L, A, T, base_anchors,
                     gt_boxes, gt_offsets, sum_g, assigned, pos_inds, inds_stride, num, nm, pos_gt, pos_delta);
  AS_CHECK_LAUNCH("rpn_targets");
  return AS_OK;
}
