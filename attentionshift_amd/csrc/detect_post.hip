// Test-time post-processing of the RoI head for gfx950: greedy NMS and the mask paste.
//
//   as_nms          mmcv.ops.nms as called by mmdet/core/post_processing/bbox_nms.py:84 (greedy, IoU without the +1
//                   offset).  Two launches: a 64 x 64-box bit mask of "column box overlaps row box" over the upper
//                   triangle, then one wave that walks the boxes in score order and compacts the kept positions.
//   as_paste_masks  mae_mask_head_pointSup.py:277-375, 411-480 (get_seg_masks / _do_paste_mask): the class channel of
//                   every RoI mask, sigmoid, bilinear resample onto the image grid of its box, threshold -- one pass that
//                   writes only the [n,H,W] result (no sampling grid, no fp32 image unless asked for).
//
// This file is compiled with -ffp-contract=off: the IoU below must round exactly like the ATen ops of
// assign.bbox_overlaps (separate multiply / add / subtract, correctly rounded divide), so that the kept set equals the
// host route's on every input, ties and IoU == threshold included.
#include "common.h"

namespace {

// torch.max / torch.min / clamp propagate NaN (fmaxf / fminf drop it)

constexpr int NMS_WAVES = 4;          // column blocks per workgroup of the mask kernel

// grid (ceil(nb / NMS_WAVES), nb), nb = ceil(n / 64); wave wv of workgroup (bx, rb) owns the block pair
// (rb, cb = bx * NMS_WAVES + wv): lane t builds mask[rb*64 + t][cb], bit j = (col > row && IoU(row, col) > thr) with
// col = cb*64 + j.  Only cb >= rb is computed (and later read).
__global__ __launch_bounds__(64 * NMS_WAVES) void nms_mask_kernel(const float4* __restrict__ boxes, int n, int nb, float thr,
                                                                  unsigned long long* __restrict__ mask) {
  __shared__ float4 cbox[NMS_WAVES][64];
  __shared__ float carea[NMS_WAVES][64];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  const int rb = blockIdx.y, cb = blockIdx.x * NMS_WAVES + wv;
  const bool live = cb >= rb && cb < nb;
  const int col0 = cb * 64;
  if (live && col0 + t < n) {
    const float4 b = boxes[col0 + t];
    cbox[wv][t] = b;
    carea[wv][t] = (b.z - b.x) * (b.w - b.y);
  }
  __syncthreads();
  const int row = rb * 64 + t;
  if (!live || row >= n) return;
  const float4 a = boxes[row];
  const float area_a = (a.z - a.x) * (a.w - a.y);
  const int ncol = min(64, n - col0);
  unsigned long long word = 0;
  for (int j = 0; j < ncol; ++j) {
    const float4 b = cbox[wv][j];
    const float w = nan_max(nan_min(a.z, b.z) - nan_max(a.x, b.x), 0.0f);
    const float h = nan_max(nan_min(a.w, b.w) - nan_max(a.y, b.y), 0.0f);
    const float inter = w * h;
    const float uni = nan_max((area_a + carea[wv][j]) - inter, 1e-12f);
    const float iou = __fdiv_rn(inter, uni);
    if (col0 + j > row && iou > thr) word |= 1ull << j;
  }
  mask[(size_t)row * nb + cb] = word;
}

__device__ __forceinline__ unsigned long long bcast64(unsigned long long v) {      // lane 0's value as a wave-uniform scalar
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// One wave.  remv (the "removed" bit set, one bit per box) lives in LDS, lane l owning words l, l + 64, ...  Per 64-box
// block: the chain inside the block is resolved on the scalar unit from the diagonal mask words (lane t holds row t's;
// v_readlane fetches the word of each box that is kept), then the mask rows of the kept boxes are OR-ed into the words of
// the blocks still to come (lanes read consecutive words: coalesced).
__global__ __launch_bounds__(64) void nms_reduce_kernel(const unsigned long long* __restrict__ mask, int n, int nb, int max_keep,
                                                        long long* __restrict__ keep_idx, int* __restrict__ count_out) {
  __shared__ unsigned long long remv[1024];                // n <= 65535 -> nb <= 1024
  const int lane = threadIdx.x;
  for (int w = lane; w < nb; w += 64) remv[w] = 0;
  __syncthreads();
  int count = 0;
  for (int blk = 0; blk < nb; ++blk) {
    const int row = blk * 64 + lane;
    const unsigned long long diag = row < n ? mask[(size_t)row * nb + blk] : 0ull;
    const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
    const int nrow = min(64, n - blk * 64);
    const unsigned long long valid = nrow == 64 ? ~0ull : ((1ull << nrow) - 1);
    unsigned long long alive = ~bcast64(remv[blk]) & valid, keepw = 0;
    int kept = 0;
    while (alive) {
      const int t = __builtin_ctzll(alive);
      keepw |= 1ull << t;
      ++kept;
      if (max_keep > 0 && count + kept == max_keep) break;
      const unsigned lo = __builtin_amdgcn_readlane(dlo, t), hi = __builtin_amdgcn_readlane(dhi, t);   // (the builtin returns int)
      alive &= ~((((unsigned long long)hi << 32) | lo) | (1ull << t));
    }
    if ((keepw >> lane) & 1ull) keep_idx[count + __builtin_popcountll(keepw & ((1ull << lane) - 1))] = row;
    count += kept;
    if (max_keep > 0 && count >= max_keep) break;
    // remv[w] |= mask[kept row][w] for the later blocks, four kept rows per trip so that their loads overlap
    for (int w = blk + 1 + lane; w < nb; w += 64) {
      unsigned long long acc = 0, left = keepw;
      while (left) {
        int t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          t[u] = left ? __builtin_ctzll(left) : -1;
          if (left) left &= left - 1;
        }
        unsigned long long v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = t[u] >= 0 ? mask[(size_t)(blk * 64 + t[u]) * nb + w] : 0ull;
        acc |= (v[0] | v[1]) | (v[2] | v[3]);
      }
      remv[w] |= acc;
    }
    __syncthreads();
  }
  if (lane == 0) *count_out = count;
}

// --------------------------------------------------------------------------------------------------------------------
// mask paste
// --------------------------------------------------------------------------------------------------------------------
constexpr int PM_NT = 256;
constexpr int PM_SPAN = 8192;          // output pixels per workgroup (rounded to whole rows); measured best of 2048 .. 131072

template <int MODE> struct PasteOut;
template <> struct PasteOut<0> {
  typedef float elem;
  static constexpr int N = 4;
  static __device__ __forceinline__ float cvt(float v, float) { return v; }
};
template <> struct PasteOut<1> {
  typedef uint8_t elem;
  static constexpr int N = 16;
  static __device__ __forceinline__ uint8_t cvt(float v, float thr) { return v >= thr ? 1 : 0; }
};
template <> struct PasteOut<2> {
  typedef uint8_t elem;
  static constexpr int N = 16;
  static __device__ __forceinline__ uint8_t cvt(float v, float) { return (uint8_t)(int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f); }
};

// grid (ceil(H / rows), n): one workgroup = `rows` image rows of one detection = one contiguous span of the output.  The
// detection's h x w channel is staged in LDS (through the sigmoid when asked).  The span is cut into 16-byte pieces of
// the OUTPUT ADDRESS (W is arbitrary, so a row does not start aligned): a lane computes the 16 / 4 pixels of a piece and
// stores them with one 16-byte store; the ragged head and tail of the span go out element by element.
template <int MODE>
__global__ __launch_bounds__(PM_NT) void paste_kernel(const float* __restrict__ src, const long long* __restrict__ labels,
                                                      const float4* __restrict__ boxes, typename PasteOut<MODE>::elem* __restrict__ out,
                                                      int K, int h, int w, int H, int W, int rows, int apply_sigmoid, float thr) {
  typedef PasteOut<MODE> O;
  typedef typename O::elem elem;
  extern __shared__ float tile[];                          // [h][w]
  const int i = blockIdx.y, y_begin = blockIdx.x * rows, y_end = min(H, y_begin + rows);
  const float4 box = boxes[i];
  const float bw = box.z - box.x, bh = box.w - box.y;
  const long long ch = labels ? labels[i] : 0;
  const float fw = (float)w, fh = (float)h;
  // sample row of image row y: the arithmetic of inference.paste_masks + grid_sample(align_corners=False)
  auto src_coord = [](int p, float p0, float extent, float size) {
    const float g = (((float)p + 0.5f) - p0) / extent * 2.0f - 1.0f;
    return ((g + 1.0f) * size - 1.0f) / 2.0f;
  };
  // the workgroup is live when its detection has a proper box and channel and one of its rows samples inside (-1, h)
  bool live = bw > 0.0f && bh > 0.0f && ch >= 0 && ch < K;
  if (live) {
    const float iy_a = src_coord(y_begin, box.y, bh, fh), iy_b = src_coord(y_end - 1, box.y, bh, fh);   // increasing in y
    live = iy_b > -1.0f && iy_a < fh;
  }
  if (live) {
    const float* s = src + ((size_t)i * K + (size_t)ch) * h * w;
    for (int k = threadIdx.x; k < h * w; k += PM_NT) {
      const float v = s[k];
      tile[k] = apply_sigmoid ? 1.0f / (1.0f + expf(-v)) : v;
    }
  }
  __syncthreads();

  // per image row: its sample row iy, and whether any pixel of it can be inside (most rows of an image lie outside a
  // detection's box: they cost no arithmetic beyond this)
  auto row_setup = [&](int y, float& iy) -> bool {
    iy = src_coord(y, box.y, bh, fh);
    return live && iy > -1.0f && iy < fh;
  };
  auto sample = [&](int x, float iy, bool row_live) -> float {
    if (!row_live) return 0.0f;
    const float ix = src_coord(x, box.x, bw, fw);
    if (!(ix > -1.0f && ix < fw)) return 0.0f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;                  // in [-1, w-1] x [-1, h-1]
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix, wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    const bool xl = x0 >= 0, xr = x0 + 1 < w, yt = y0 >= 0, yb = y0 + 1 < h;
    float v = 0.0f;
    if (xl && yt) v += tile[y0 * w + x0] * (wx0 * wy0);
    if (xr && yt) v += tile[y0 * w + x0 + 1] * (wx1 * wy0);
    if (xl && yb) v += tile[(y0 + 1) * w + x0] * (wx0 * wy1);
    if (xr && yb) v += tile[(y0 + 1) * w + x0 + 1] * (wx1 * wy1);
    return v;
  };

  const int len = (y_end - y_begin) * W;                   // pixels of this span
  elem* span = out + ((size_t)i * H + y_begin) * W;
  const int lead = (int)((reinterpret_cast<uintptr_t>(span) & 15) / sizeof(elem));   // elements since the last 16-byte line
  const int npieces = (len + lead + O::N - 1) / O::N;
  for (int c = threadIdx.x; c < npieces; c += PM_NT) {
    const int q0 = c * O::N - lead;                        // first pixel of the piece, relative to the span
    const int qa = max(q0, 0);
    int y = y_begin + qa / W, x = qa % W;
    float iy;
    bool row_live = row_setup(y, iy);
    if (q0 >= 0 && q0 + O::N <= len) {
      elem e[O::N];
#pragma unroll
      for (int k = 0; k < O::N; ++k) {
        e[k] = O::cvt(sample(x, iy, row_live), thr);
        if (++x == W) { x = 0; row_live = row_setup(++y, iy); }
      }
      uint4 pk;
      memcpy(&pk, e, 16);
      *reinterpret_cast<uint4*>(span + q0) = pk;
    } else {
      const int qe = min(q0 + O::N, len);
      for (int q = qa; q < qe; ++q) {
        span[q] = O::cvt(sample(x, iy, row_live), thr);
        if (++x == W) { x = 0; row_live = row_setup(++y, iy); }
      }
    }
  }
}

}  // namespace

extern "C" size_t as_nms_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return (size_t)n * (size_t)as_ceil_div(n, 64) * 8;
}

extern "C" int as_nms(const float* boxes_sorted, int n, float iou_thr, int max_keep, long long* keep_idx, int* count,
                      void* workspace, size_t workspace_bytes, as_stream_t stream) {
  AS_REQUIRE(n >= 0, AS_E_BADARG, "as_nms: n < 0");
  AS_REQUIRE(count, AS_E_BADARG, "as_nms: null pointer");
  AS_REQUIRE(n == 0 || (boxes_sorted && keep_idx && workspace), AS_E_BADARG, "as_nms: null pointer");
  AS_REQUIRE(n <= 65535, AS_E_UNSUPPORTED, "as_nms: n = %d > 65535 (the pair mask would exceed 512 MB)", n);
  AS_REQUIRE(workspace_bytes >= as_nms_workspace_bytes(n), AS_E_WORKSPACE, "as_nms: workspace of %zu bytes, %zu needed",
             workspace_bytes, as_nms_workspace_bytes(n));
  AS_REQUIRE(n == 0 || (reinterpret_cast<uintptr_t>(boxes_sorted) & 15) == 0, AS_E_BADARG, "as_nms: boxes not 16-byte aligned");
  AS_REQUIRE(n == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, AS_E_BADARG, "as_nms: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int nb = as_ceil_div(n, 64);
  unsigned long long* mask = static_cast<unsigned long long*>(workspace);
  if (n > 0)
    hipLaunchKernelGGL(nms_mask_kernel, dim3(as_ceil_div(nb, NMS_WAVES), nb), dim3(64 * NMS_WAVES), 0, s,
                       reinterpret_cast<const float4*>(boxes_sorted), n, nb, iou_thr, mask);
  hipLaunchKernelGGL(nms_reduce_kernel, dim3(1), dim3(64), 0, s, mask, n, nb, max_keep, keep_idx, count);
  AS_CHECK_LAUNCH("nms");
  return AS_OK;
}

extern "C" int as_paste_masks(const float* src, const long long* labels, const float* boxes, void* out, int n, int K, int h,
                              int w, int H, int W, int apply_sigmoid, int out_mode, float thr, as_stream_t stream) {
  AS_REQUIRE(n >= 0 && K > 0 && h > 0 && w > 0 && H >= 0 && W >= 0, AS_E_BADARG, "as_paste_masks: bad sizes");
  AS_REQUIRE(out_mode >= 0 && out_mode <= 2, AS_E_BADARG, "as_paste_masks: out_mode %d (0 fp32, 1 threshold, 2 levels)", out_mode);
  if (n == 0 || H == 0 || W == 0) return AS_OK;
  AS_REQUIRE(src && boxes && out, AS_E_BADARG, "as_paste_masks: null pointer");
  AS_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0, AS_E_BADARG,
             "as_paste_masks: boxes not 16-byte / out not 4-byte aligned");
  AS_REQUIRE((size_t)h * w <= 16384, AS_E_UNSUPPORTED, "as_paste_masks: a %d x %d mask does not fit the 64 KB LDS tile", h, w);
  AS_REQUIRE((size_t)H * W <= 0x7fffffff && n <= 65535, AS_E_UNSUPPORTED, "as_paste_masks: image or batch too large");
  hipStream_t s = (hipStream_t)stream;
  const int rows = W >= PM_SPAN ? 1 : PM_SPAN / W;
  const dim3 grid(as_ceil_div(H, rows), n), block(PM_NT);
  const size_t lds = (size_t)h * w * sizeof(float);
  if (out_mode == 0)
    hipLaunchKernelGGL(paste_kernel<0>, grid, block, lds, s, src, labels, reinterpret_cast<const float4*>(boxes),
                       static_cast<float*>(out), K, h, w, H, W, rows, apply_sigmoid, thr);
  else if (out_mode == 1)
    hipLaunchKernelGGL(paste_kernel<1>, grid, block, lds, s, src, labels, reinterpret_cast<const float4*>(boxes),
                       static_cast<uint8_t*>(out), K, h, w, H, W, rows, apply_sigmoid, thr);
  else
    hipLaunchKernelGGL(paste_kernel<2>, grid, block, lds, s, src, labels, reinterpret_cast<const float4*>(boxes),
                       static_cast<uint8_t*>(out), K, h, w, H, W, rows, apply_sigmoid, thr);
  AS_CHECK_LAUNCH("paste_masks");
  return AS_OK;
}
