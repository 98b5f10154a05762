// RPN proposal candidates for gfx950: what mmdet/models/dense_heads/rpn_head.py:82-236 (RPNHead._get_bboxes) does before
// its batched_nms, without an anchor tensor, a full sort or a gather per level.
//
//   as_rpn_candidates   three launches for all B x L (image, level) pairs:
//     1. rpn_select_kernel   one workgroup per (image, level).  A histogram of the keys' first 11 bits finds the bin that
//                            holds the k-th key; a second read takes the keys of the bins before it and sorts those of
//                            the bin itself in LDS (two reads of every logit).  When that bin holds more than 4096 keys
//                            (ties, a very narrow distribution) the radix select goes on over the other 11 + 10 bits and
//                            one ordered pass collects the survivors, ties at the cut going to the lowest candidate
//                            indices (four reads).  A bitonic sort of the k survivors in LDS ends both.
//     2. rpn_decode_kernel   one thread per survivor: its place in the image's total order by binary searches in the
//                            other levels' sorted lists, its anchor from (level, index), delta2bbox, the sigmoid.
//     3. rpn_finish_kernel   one workgroup per image: the minimum-size filter as an ordered compaction, M = the largest
//                            surviving coordinate, the boxes offset by level * (M + 1) for as_nms.
//
// The total order is (logit descending, level ascending, candidate index ascending) as ONE 64-bit key per candidate:
//   bits 63..32  ~u, u = the order-preserving unsigned image of the logit (-0.0 folded onto +0.0, any NaN = 0xffffffff, so
//                a NaN ranks above +inf as torch.sort(descending=True) ranks it)
//   bits 30..28  the level          bits 27..0  the candidate index i = (y * W + x) * A + a
// Keys of one image are distinct, so ascending key order is the total order and nothing depends on thread timing.
//
// This file is compiled with -ffp-contract=off: apart from expf every step of the decode rounds like the ATen ops of
// bbox_loss.delta2bbox (separate multiply / add, correctly rounded divide).
#include "common.h"

namespace {

constexpr int RPN_NT = 1024;           // threads of the select and finish kernels (16 waves)
constexpr int RPN_WAVES = RPN_NT / 64;
constexpr int RPN_MAX_L = 8;
constexpr int RPN_MAX_K = 2048;        // survivors per (image, level): one bitonic sort of 16 KB in LDS
constexpr int RPN_MAX_C = RPN_MAX_L * RPN_MAX_K;
constexpr int RPN_IDX_BITS = 28;
constexpr int RPN_BINS = 2048;
constexpr int RPN_CAND = 4096;         // keys of the histogram bin that holds the cut, when they fit: sorted in 32 KB of LDS
constexpr int RPN_UNROLL = 8;          // independent loads per thread and trip of a scan
constexpr int RPN_DEC_NT = 256;

struct RpnLevels {
  const float* cls[RPN_MAX_L];
  const float* reg[RPN_MAX_L];
  int H[RPN_MAX_L], W[RPN_MAX_L], sx[RPN_MAX_L], sy[RPN_MAX_L];
  int k[RPN_MAX_L];                    // survivors of the level
  int off[RPN_MAX_L];                  // their first slot among the image's C
};
struct RpnNorm {
  float mean[4], std[4];
};

// ascending in this = descending in the logit
__device__ __forceinline__ unsigned desc_key(float v) {
  if (v != v) return 0u;
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

__device__ __forceinline__ unsigned long long make_key(unsigned dk, int level, int i) {
  return ((unsigned long long)dk << 32) | ((unsigned long long)level << RPN_IDX_BITS) | (unsigned)i;
}

// logit of candidate i of one image's level: cls[a][y][x], i = (y * W + x) * A + a
__device__ __forceinline__ float cand_logit(const float* __restrict__ cls, int i, int A, int HW) {
  const int p = i / A, a = i - p * A;
  return cls[(size_t)a * HW + p];
}

// f(key, i) for every candidate of one image's level, in no particular order: plane by plane (coalesced, no division),
// RPN_UNROLL independent loads in flight per thread
template <typename F>
__device__ __forceinline__ void scan_planes(const float* __restrict__ cls, int A, int HW, int tid, F f) {
  for (int a = 0; a < A; ++a) {
    const float* pl = cls + (size_t)a * HW;
    for (int base = 0; base < HW; base += RPN_NT * RPN_UNROLL) {
      float v[RPN_UNROLL];
#pragma unroll
      for (int u = 0; u < RPN_UNROLL; ++u) {
        const int p = base + u * RPN_NT + tid;
        v[u] = p < HW ? pl[p] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < RPN_UNROLL; ++u) {
        const int p = base + u * RPN_NT + tid;
        if (p < HW) f(desc_key(v[u]), p * A + a);
      }
    }
  }
}

__global__ __launch_bounds__(RPN_NT) void rpn_select_kernel(RpnLevels lv, int L, int A, int C, unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long buf[RPN_MAX_K];            // the survivors
  __shared__ unsigned long long cand[RPN_CAND];            // the candidates of the bin that holds the cut
  __shared__ unsigned hist[RPN_BINS];
  __shared__ unsigned wsum[RPN_WAVES];
  __shared__ unsigned wtot[2][RPN_WAVES];
  __shared__ unsigned sh_bin, sh_below, sh_count, cnt_less, cnt_cand;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = blockIdx.x % L, b = blockIdx.x / L;
  const int HW = lv.H[l] * lv.W[l], n = A * HW, k = lv.k[l];
  const float* cls = lv.cls[l] + (size_t)b * n;
  int P = 2;
  while (P < k) P <<= 1;
  for (int j = tid; j < P; j += RPN_NT) buf[j] = ~0ull;
  if (tid == 0) cnt_less = cnt_cand = 0;
  __syncthreads();

  // the bin of hist (digit `shift` of the keys that match prefix under himask) in which the running count reaches krem:
  // -> sh_bin, sh_below = the count of the bins before it, sh_count = its own.  Thread t owns bins 2t and 2t + 1.
  auto find_bin = [&](unsigned krem) {
    const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
    const unsigned incl_w = wave_incl_scan(h0 + h1, lane);
    if (lane == 63) wsum[wave] = incl_w;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    const unsigned incl = before + incl_w, excl = incl - (h0 + h1);
    if (excl < krem && krem <= incl) {                     // exactly one thread
      const bool first = excl + h0 >= krem;
      sh_bin = 2 * tid + (first ? 0 : 1);
      sh_below = first ? excl : excl + h0;
      sh_count = first ? h0 : h1;
    }
    __syncthreads();
  };

  if (k == n) {                                            // the level passes whole
    scan_planes(cls, A, HW, tid, [&](unsigned key, int i) { buf[i] = make_key(key, l, i); });
  } else {
    // first digit (11 bits) of the k-th smallest key
    for (int j = tid; j < RPN_BINS; j += RPN_NT) hist[j] = 0;
    __syncthreads();
    scan_planes(cls, A, HW, tid, [&](unsigned key, int) { atomicAdd(&hist[key >> 21], 1u); });
    __syncthreads();
    find_bin((unsigned)k);
    const unsigned tbin = sh_bin, nbelow = sh_below, nt = sh_count;
    unsigned krem = (unsigned)k - nbelow;                  // how many keys of bin tbin are taken, 1 <= krem <= nt
    __syncthreads();
    if (nt <= (unsigned)RPN_CAND) {
      // the usual case: the cut's bin fits in LDS.  Second and last read: keys of the bins before it are survivors, those of
      // the bin itself are sorted here (by key, then index) and the first krem of them taken.
      scan_planes(cls, A, HW, tid, [&](unsigned key, int i) {
        const unsigned bin = key >> 21;
        if (bin < tbin) {
          const unsigned slot = atomicAdd(&cnt_less, 1u);  // ends at nbelow exactly
          if (slot < nbelow) buf[slot] = make_key(key, l, i);
        } else if (bin == tbin) {
          const unsigned slot = atomicAdd(&cnt_cand, 1u);  // ends at nt exactly
          if (slot < (unsigned)RPN_CAND) cand[slot] = make_key(key, l, i);
        }
      });
      int P2 = 2;
      while (P2 < (int)nt) P2 <<= 1;
      for (int j = (int)nt + tid; j < P2; j += RPN_NT) cand[j] = ~0ull;
      __syncthreads();
      bitonic_sort<unsigned long long, RPN_NT>(cand, P2, tid);
      for (unsigned j = tid; j < krem; j += RPN_NT) buf[nbelow + j] = cand[j];
    } else {
      // many keys share the first digit (ties, or a very narrow distribution): two more digits give T = the k-th smallest
      // key and krem = how many candidates with key == T are taken; then one ordered pass collects
      unsigned prefix = tbin << 21, himask = 0x7ffu << 21;
      for (int pass = 1; pass < 3; ++pass) {
        const int shift = pass == 1 ? 10 : 0;
        const unsigned nbins = pass == 1 ? 2048u : 1024u;
        for (int j = tid; j < RPN_BINS; j += RPN_NT) hist[j] = 0;
        __syncthreads();
        scan_planes(cls, A, HW, tid, [&](unsigned key, int) {
          if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & (nbins - 1)], 1u);
        });
        __syncthreads();
        find_bin(krem);
        prefix |= sh_bin << shift;
        himask |= (nbins - 1) << shift;
        krem -= sh_below;
        __syncthreads();                                   // sh_bin / wsum / hist are rewritten by the next pass
      }
      const unsigned T = prefix;
      const unsigned nless = (unsigned)k - krem;
      // keys below T in any order (the sort follows), keys equal to T in candidate order up to krem of them
      unsigned eq_seen = 0;
      int parity = 0;
      for (int base = 0; base < n; base += RPN_NT * RPN_UNROLL) {
        float v[RPN_UNROLL];
#pragma unroll
        for (int u = 0; u < RPN_UNROLL; ++u) {
          const int i = base + u * RPN_NT + tid;
          v[u] = i < n ? cand_logit(cls, i, A, HW) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < RPN_UNROLL; ++u) {
          const int i = base + u * RPN_NT + tid;
          const bool valid = i < n;
          const unsigned key = valid ? desc_key(v[u]) : 0xffffffffu;
          if (valid && key < T) {
            const unsigned slot = atomicAdd(&cnt_less, 1u);  // ends at nless exactly
            if (slot < nless) buf[slot] = make_key(key, l, i);
          }
          if (eq_seen < krem) {                            // uniform: eq_seen is the same in every thread
            const bool eq = valid && key == T;
            const unsigned long long bal = __ballot(eq);
            const unsigned rank_w = __builtin_popcountll(bal & ((1ull << lane) - 1));
            if (lane == 0) wtot[parity][wave] = __builtin_popcountll(bal);
            __syncthreads();
            unsigned before = 0, total = 0;
            for (int w = 0; w < RPN_WAVES; ++w) {
              const unsigned c = wtot[parity][w];
              if (w < wave) before += c;
              total += c;
            }
            const unsigned r = eq_seen + before + rank_w;
            if (eq && r < krem) buf[nless + r] = make_key(key, l, i);
            eq_seen += total;
            parity ^= 1;
          }
        }
      }
    }
  }
  __syncthreads();
  bitonic_sort<unsigned long long, RPN_NT>(buf, P, tid);    // the padding (~0) stays behind the k keys
  unsigned long long* out = keys + (size_t)b * C + lv.off[l];
  for (int j = tid; j < k; j += RPN_NT) out[j] = buf[j];
}

// grid (ceil(C / RPN_DEC_NT), B)
__global__ __launch_bounds__(RPN_DEC_NT) void rpn_decode_kernel(RpnLevels lv, int L, int A, int C,
                                                                const unsigned long long* __restrict__ keys,
                                                                const float* __restrict__ base_anchors,
                                                                const float* __restrict__ img_shapes, RpnNorm nm, float max_ratio,
                                                                float4* __restrict__ st_box, float* __restrict__ st_score,
                                                                int* __restrict__ st_level, int* __restrict__ st_index) {
  const int j = blockIdx.x * RPN_DEC_NT + threadIdx.x, b = blockIdx.y;
  if (j >= C) return;
  const unsigned long long* kb = keys + (size_t)b * C;
  const unsigned long long key = kb[j];
  const int l = (int)((key >> RPN_IDX_BITS) & 7), i = (int)(key & ((1u << RPN_IDX_BITS) - 1));
  // place in the image's total order = number of keys below this one, level by level (every list is sorted)
  int rank = 0;
  const float *cls = nullptr, *reg = nullptr;
  int H = 1, W = 1, sx = 0, sy = 0;
  for (int l2 = 0; l2 < L; ++l2) {
    const unsigned long long* s = kb + lv.off[l2];
    int lo = 0, hi = lv.k[l2];
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s[mid] < key) lo = mid + 1; else hi = mid;
    }
    rank += lo;
    if (l2 == l) {
      cls = lv.cls[l2]; reg = lv.reg[l2];
      H = lv.H[l2]; W = lv.W[l2]; sx = lv.sx[l2]; sy = lv.sy[l2];
    }
  }
  const int HW = H * W;
  if (!cls || i >= A * HW || rank >= C) return;            // (cannot happen with keys written by rpn_select_kernel)
  const int p = i / A, a = i - p * A, y = p / W, x = p - y * W;
  const float logit = cls[((size_t)b * A + a) * HW + p];
  const float* rp = reg + ((size_t)b * 4 * A + 4 * a) * HW + p;
  const float d0 = rp[0] * nm.std[0] + nm.mean[0];
  const float d1 = rp[(size_t)HW] * nm.std[1] + nm.mean[1];
  float d2 = rp[(size_t)2 * HW] * nm.std[2] + nm.mean[2];
  float d3 = rp[(size_t)3 * HW] * nm.std[3] + nm.mean[3];
  d2 = nan_min(nan_max(d2, -max_ratio), max_ratio);
  d3 = nan_min(nan_max(d3, -max_ratio), max_ratio);
  const float* ba = base_anchors + ((size_t)l * A + a) * 4;
  const float shx = (float)(x * sx), shy = (float)(y * sy);
  const float ax1 = ba[0] + shx, ay1 = ba[1] + shy, ax2 = ba[2] + shx, ay2 = ba[3] + shy;
  const float px = (ax1 + ax2) * 0.5f, py = (ay1 + ay2) * 0.5f, pw = ax2 - ax1, ph = ay2 - ay1;
  const float gw = pw * expf(d2), gh = ph * expf(d3);
  const float gx = px + pw * d0, gy = py + ph * d1;
  const float ih = img_shapes[2 * b], iw = img_shapes[2 * b + 1];
  float4 box;
  box.x = nan_min(nan_max(gx - gw * 0.5f, 0.0f), iw);
  box.y = nan_min(nan_max(gy - gh * 0.5f, 0.0f), ih);
  box.z = nan_min(nan_max(gx + gw * 0.5f, 0.0f), iw);
  box.w = nan_min(nan_max(gy + gh * 0.5f, 0.0f), ih);
  const size_t o = (size_t)b * C + rank;
  st_box[o] = box;
  st_score[o] = __fdiv_rn(1.0f, 1.0f + expf(-logit));
  st_level[o] = l;
  st_index[o] = i;
}

// one workgroup per image
__global__ __launch_bounds__(RPN_NT) void rpn_finish_kernel(int C, float min_size, const float4* __restrict__ st_box,
                                                            const float* __restrict__ st_score, const int* __restrict__ st_level,
                                                            const int* __restrict__ st_index, float4* __restrict__ cand_box,
                                                            float4* __restrict__ cand_nms_box, float* __restrict__ cand_score,
                                                            int* __restrict__ cand_level, int* __restrict__ cand_index,
                                                            int* __restrict__ cand_count) {
  __shared__ unsigned wtot[2][RPN_WAVES];
  __shared__ float wmax[RPN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const size_t o = (size_t)b * C;
  float m = -INFINITY;
  unsigned kept = 0;
  int parity = 0;
  for (int base = 0; base < C; base += RPN_NT) {
    const int j = base + tid;
    bool ok = j < C;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
      box = st_box[o + j];
      if (min_size > 0.0f) ok = (box.z - box.x) >= min_size && (box.w - box.y) >= min_size;
    }
    const unsigned long long bal = __ballot(ok);
    const unsigned rank_w = __builtin_popcountll(bal & ((1ull << lane) - 1));
    if (lane == 0) wtot[parity][wave] = __builtin_popcountll(bal);
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int w = 0; w < RPN_WAVES; ++w) {
      const unsigned c = wtot[parity][w];
      if (w < wave) before += c;
      total += c;
    }
    if (ok) {
      const size_t q = o + kept + before + rank_w;
      cand_box[q] = box;
      cand_score[q] = st_score[o + j];
      cand_level[q] = st_level[o + j];
      cand_index[q] = st_index[o + j];
      m = nan_max(m, nan_max(nan_max(box.x, box.y), nan_max(box.z, box.w)));
    }
    kept += total;
    parity ^= 1;
  }
  // M, NaN propagating like Tensor.max()
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = nan_max(m, __shfl_xor(m, s));
  if (lane == 0) wmax[wave] = m;
  __syncthreads();                                         // also orders this workgroup's cand_* stores before the reads below
  float M = wmax[0];
  for (int w = 1; w < RPN_WAVES; ++w) M = nan_max(M, wmax[w]);
  const float step = M + 1.0f;
  for (int j = tid; j < (int)kept; j += RPN_NT) {
    const float4 box = cand_box[o + j];
    const float off = (float)cand_level[o + j] * step;
    cand_nms_box[o + j] = make_float4(box.x + off, box.y + off, box.z + off, box.w + off);
  }
  if (tid == 0) cand_count[b] = (int)kept;
}

// -> C, or -1 when a level is malformed; fills k / off
long long rpn_plan(const as_rpn_level* levels, int L, int A, int nms_pre, RpnLevels* lv, bool* too_big) {
  long long C = 0;
  *too_big = false;
  for (int l = 0; l < L; ++l) {
    if (levels[l].H <= 0 || levels[l].W <= 0) return -1;
    const long long n = (long long)A * levels[l].H * levels[l].W;
    const long long k = (nms_pre > 0 && nms_pre < n) ? nms_pre : n;
    if (n >= (1ll << RPN_IDX_BITS) || k > RPN_MAX_K) *too_big = true;
    if (lv) {
      lv->cls[l] = levels[l].cls; lv->reg[l] = levels[l].reg;
      lv->H[l] = levels[l].H; lv->W[l] = levels[l].W;
      lv->sx[l] = levels[l].stride_x; lv->sy[l] = levels[l].stride_y;
      lv->k[l] = (int)(k > RPN_MAX_K ? RPN_MAX_K : k);
      lv->off[l] = (int)(C > RPN_MAX_C ? RPN_MAX_C : C);
    }
    C += k;
  }
  return C;
}

}  // namespace

extern "C" size_t as_rpn_candidates_workspace_bytes(int B, int C) {
  if (B <= 0 || C <= 0) return 0;
  return (size_t)36 * (size_t)B * (size_t)C;
}

extern "C" int as_rpn_candidates(const as_rpn_level* levels, int L, int B, int A, const float* base_anchors, const float* img_shapes,
                                 int nms_pre, float min_bbox_size, const float* means_stds, float max_ratio, int C, float* cand_box,
                                 float* cand_nms_box, float* cand_score, int32_t* cand_level, int32_t* cand_index,
                                 int32_t* cand_count, void* workspace, size_t workspace_bytes, as_stream_t stream) {
  AS_REQUIRE(levels && means_stds, AS_E_BADARG, "as_rpn_candidates: null host pointer");
  AS_REQUIRE(L >= 1 && L <= RPN_MAX_L, AS_E_BADARG, "as_rpn_candidates: L = %d outside 1 .. %d", L, RPN_MAX_L);
  AS_REQUIRE(A >= 1 && B >= 0, AS_E_BADARG, "as_rpn_candidates: A = %d, B = %d", A, B);
  for (int l = 0; l < L; ++l)
    AS_REQUIRE(levels[l].cls && levels[l].reg, AS_E_BADARG, "as_rpn_candidates: null pointer in level %d", l);
  RpnLevels lv;
  memset(&lv, 0, sizeof(lv));
  bool too_big = false;
  const long long Cx = rpn_plan(levels, L, A, nms_pre, &lv, &too_big);
  AS_REQUIRE(Cx >= 0, AS_E_BADARG, "as_rpn_candidates: a level with H <= 0 or W <= 0");
  AS_REQUIRE((long long)C == Cx, AS_E_BADARG, "as_rpn_candidates: C = %d, the levels and nms_pre give %lld", C, Cx);
  AS_REQUIRE(!too_big && Cx <= RPN_MAX_C, AS_E_UNSUPPORTED,
             "as_rpn_candidates: more than %d survivors in a level, %d in all, or a level of 2^%d candidates", RPN_MAX_K, RPN_MAX_C,
             RPN_IDX_BITS);
  for (int l = 0; l < L; ++l)
    AS_REQUIRE(levels[l].stride_x >= 0 && levels[l].stride_y >= 0 &&
                   (long long)levels[l].stride_x * levels[l].W < (1 << 24) && (long long)levels[l].stride_y * levels[l].H < (1 << 24),
               AS_E_BADARG, "as_rpn_candidates: stride of level %d negative or its shifts not exact in fp32", l);
  if (B == 0) return AS_OK;
  AS_REQUIRE(base_anchors && img_shapes && cand_box && cand_nms_box && cand_score && cand_level && cand_index && cand_count &&
                 workspace,
             AS_E_BADARG, "as_rpn_candidates: null pointer");
  AS_REQUIRE(B <= 65535, AS_E_UNSUPPORTED, "as_rpn_candidates: B = %d > 65535", B);
  AS_REQUIRE(workspace_bytes >= as_rpn_candidates_workspace_bytes(B, C), AS_E_WORKSPACE,
             "as_rpn_candidates: workspace of %zu bytes, %zu needed", workspace_bytes, as_rpn_candidates_workspace_bytes(B, C));
  AS_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(cand_box) |
               reinterpret_cast<uintptr_t>(cand_nms_box)) & 15) == 0,
             AS_E_BADARG, "as_rpn_candidates: workspace / cand_box / cand_nms_box not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t BC = (size_t)B * C;
  char* w = static_cast<char*>(workspace);
  float4* st_box = reinterpret_cast<float4*>(w);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(w + 16 * BC);
  float* st_score = reinterpret_cast<float*>(w + 24 * BC);
  int* st_level = reinterpret_cast<int*>(w + 28 * BC);
  int* st_index = reinterpret_cast<int*>(w + 32 * BC);
  RpnNorm nm;
  for (int c = 0; c < 4; ++c) {
    nm.mean[c] = means_stds[c];
    nm.std[c] = means_stds[4 + c];
  }
  hipLaunchKernelGGL(rpn_select_kernel, dim3(B * L), dim3(RPN_NT), 0, s, lv, L, A, C, keys);
  hipLaunchKernelGGL(rpn_decode_kernel, dim3(as_ceil_div(C, RPN_DEC_NT), B), dim3(RPN_DEC_NT), 0, s, lv, L, A, C, keys, base_anchors,
                     img_shapes, nm, max_ratio, st_box, st_score, st_level, st_index);
  hipLaunchKernelGGL(rpn_finish_kernel, dim3(B), dim3(RPN_NT), 0, s, C, min_bbox_size, st_box, st_score, st_level, st_index,
                     reinterpret_cast<float4*>(cand_box), reinterpret_cast<float4*>(cand_nms_box), cand_score, cand_level, cand_index,
                     cand_count);
  AS_CHECK_LAUNCH("rpn_candidates");
  return AS_OK;
}
