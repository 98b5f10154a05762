// COCO run-length encoding of the test-time masks for gfx950, so that only the encoded strings leave the device.
//
//   as_rle_count / as_rle_encode   mmdet/core/mask/utils.py:36-63 (encode_mask_results, called on every simple_test result by
//                                  mmdet/apis/test.py:60,100): pycocotools' rleEncode + rleToString of every [H,W] mask in
//                                  Fortran order.
//
// Input: masks [n,H,W] bytes, row-major (what as_paste_masks writes in mode 1).  ANY NONZERO BYTE COUNTS AS 1.
//
// The format.  Pixels are read column by column, p = x * H + y.  The counts alternate between runs of 0 and runs of 1 and
// start with a run of 0, so a mask with T value changes has T + 1 counts.  Pixel (x, y) is a value change when it differs
// from (x, y-1), from (x-1, H-1) when y = 0, from 0 when it is pixel (0, 0) -- so the column-major order needs no
// transpose: a lane that owns columns and walks down the rows sees every change while the wave reads row-contiguous bytes.
//
//   rle_count_kernel   a wave = RLE_ROWS rows x RLE_WG_COLS columns of one detection, a lane = RLE_LANE_COLS adjacent columns
//                      (one 8-byte load per row); changes per (detection, row segment, column) as bytes
//   rle_scan_kernel    one workgroup per detection: exclusive scan of those counts in column-major order (column, then
//                      segment) -> the offset of every (segment, column) cell among the detection's changes, and the total
//   rle_base_kernel    exclusive scan of the totals over the detections -> where each detection's positions start
//   rle_fill_kernel    the walk of rle_count_kernel again; every change writes its position p at its cell's offset, in row
//                      order inside the cell: the order is a function of the scan alone (no atomics)
//   rle_string_kernel  one workgroup per detection: counts = position differences, x = cnt[i] - cnt[i-2] for i > 2, 5-bit
//                      groups low first with the continuation bit 0x20 and the offset 48, byte offsets by a workgroup scan
#include "common.h"

namespace {

constexpr int RLE_NT = 256;
constexpr int RLE_WAVES = RLE_NT / 64;                 // row segments per workgroup
constexpr int RLE_ROWS = 64;                           // rows per segment = per wave (<= 255: a cell's count is a byte)
constexpr int RLE_LANE_COLS = 8;                       // columns per lane
constexpr int RLE_WG_COLS = 64 * RLE_LANE_COLS;        // columns per workgroup
constexpr int RLE_STR_ITEMS = 4;                       // counts per thread and trip of the string kernel

typedef unsigned long long u64;

// eight mask bytes -> eight 0 / 1 bytes
__device__ __forceinline__ u64 norm8(u64 v) {
  v |= v >> 4;
  v |= v >> 2;
  v |= v >> 1;
  return v & 0x0101010101010101ull;
}

// columns xs .. xs+7 of a row as 0 / 1 bytes; a column outside [0, W) reads as 0 (xs = -1 at the seam of column 0)
__device__ __forceinline__ u64 load8(const uint8_t* __restrict__ row, long long xs, int W) {
  u64 v = 0;
  if (xs >= 0 && xs <= (long long)W - 8) {
    memcpy(&v, row + xs, 8);
  } else {
    for (int k = 0; k < 8; ++k) {
      const long long x = xs + k;
      if (x >= 0 && x < W) v |= (u64)row[x] << (8 * k);
    }
  }
  return norm8(v);
}

// what the cell (detection d, segment s, columns x0 .. x0+7) of this lane is, or false when the lane has nothing to do
struct Cell {
  const uint8_t* m;      // the detection's mask
  long long x0;
  int s, y0, ny;
  size_t cell;           // index of (d, s, x0) in the [n][S][W] arrays
};
__device__ __forceinline__ bool rle_cell(const uint8_t* __restrict__ masks, int H, int W, int S, int colblocks, Cell& c) {
  const int d = blockIdx.y, bx = blockIdx.x % colblocks, by = blockIdx.x / colblocks;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  c.s = by * RLE_WAVES + wv;
  c.x0 = (long long)bx * RLE_WG_COLS + lane * RLE_LANE_COLS;
  if (c.s >= S || c.x0 >= W) return false;
  c.m = masks + (size_t)d * H * W;
  c.y0 = c.s * RLE_ROWS;
  c.ny = min(H - c.y0, RLE_ROWS);
  c.cell = ((size_t)d * S + c.s) * W + c.x0;
  return true;
}
// the pixels the first row of the cell is compared with: the row above, or the last row one column to the left
// (a column past W has no changes: its byte stays 0 like the bytes load8 gives it in the rows of the cell)
__device__ __forceinline__ u64 rle_prev(const Cell& c, int H, int W) {
  if (c.y0 > 0) return load8(c.m + (size_t)(c.y0 - 1) * W, c.x0, W);
  const u64 seam = load8(c.m + (size_t)(H - 1) * W, c.x0 - 1, W);
  const long long ncol = (long long)W - c.x0;            // > 0
  return ncol >= 8 ? seam : seam & ((1ull << (8 * ncol)) - 1);
}

// grid (colblocks * ceil(S / RLE_WAVES), n)
__global__ __launch_bounds__(RLE_NT) void rle_count_kernel(const uint8_t* __restrict__ masks, int H, int W, int S, int colblocks,
                                                           uint8_t* __restrict__ cnt) {
  Cell c;
  if (!rle_cell(masks, H, W, S, colblocks, c)) return;
  u64 prev = rle_prev(c, H, W), acc = 0;               // acc: eight byte counters, each <= RLE_ROWS
  const uint8_t* row = c.m + (size_t)c.y0 * W;
  const bool full = c.x0 <= (long long)W - 8;
  if (full) {
    row += c.x0;
#pragma unroll 8
    for (int y = 0; y < c.ny; ++y) {
      u64 v;
      memcpy(&v, row, 8);
      row += W;
      const u64 cur = norm8(v);
      acc += cur ^ prev;
      prev = cur;
    }
    memcpy(cnt + c.cell, &acc, 8);
  } else {
    for (int y = 0; y < c.ny; ++y) {
      const u64 cur = load8(row, c.x0, W);
      row += W;
      acc += cur ^ prev;
      prev = cur;
    }
    for (int k = 0; k < 8 && c.x0 + k < W; ++k) cnt[c.cell + k] = (uint8_t)(acc >> (8 * k));
  }
}

// exclusive scan over the RLE_NT threads of a workgroup; sm holds RLE_WAVES values
template <typename T> __device__ __forceinline__ T block_excl_scan(T v, T& total, T* sm) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const T inc = wave_incl_scan(v, lane);
  __syncthreads();                                     // the previous call's reads of sm are done
  if (lane == 63) sm[wv] = inc;
  __syncthreads();
  T before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < RLE_WAVES; ++w) {
    const T t = sm[w];
    if (w < wv) before += t;
    tot += t;
  }
  total = tot;
  return before + inc - v;
}

// grid n.  A thread takes a column: its changes over the segments, a workgroup scan over 256 columns at a time with a
// carry, then the running offset of every (segment, column) cell.
__global__ __launch_bounds__(RLE_NT) void rle_scan_kernel(const uint8_t* __restrict__ cnt, uint32_t* __restrict__ segoff,
                                                          uint32_t* __restrict__ totals, int S, int W) {
  __shared__ uint32_t sm[RLE_WAVES];
  const size_t base = (size_t)blockIdx.x * S * W;
  const uint8_t* c = cnt + base;
  uint32_t* o = segoff + base;
  uint32_t carry = 0;
  for (long long xb = 0; xb < W; xb += RLE_NT) {
    const long long x = xb + threadIdx.x;
    uint32_t colsum = 0;
    if (x < W)
      for (int s = 0; s < S; ++s) colsum += c[(size_t)s * W + x];
    uint32_t total;
    uint32_t run = carry + block_excl_scan(colsum, total, sm);
    if (x < W)
      for (int s = 0; s < S; ++s) {
        o[(size_t)s * W + x] = run;
        run += c[(size_t)s * W + x];
      }
    carry += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// one workgroup: base[d] = sum of totals[0 .. d), base[n] = all
__global__ __launch_bounds__(RLE_NT) void rle_base_kernel(const uint32_t* __restrict__ totals, int n, u64* __restrict__ base) {
  __shared__ u64 sm[RLE_WAVES];
  u64 carry = 0;
  for (int d0 = 0; d0 < n; d0 += RLE_NT) {
    const int d = d0 + threadIdx.x;
    u64 total;
    const u64 excl = block_excl_scan<u64>(d < n ? totals[d] : 0, total, sm);
    if (d < n) base[d] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) base[n] = carry;
}

// the grid of rle_count_kernel.  pos_cap: elements of pos (a store past it is dropped: the totals are the caller's word)
__global__ __launch_bounds__(RLE_NT) void rle_fill_kernel(const uint8_t* __restrict__ masks, int H, int W, int S, int colblocks,
                                                          const uint32_t* __restrict__ segoff, const u64* __restrict__ base,
                                                          uint32_t* __restrict__ pos, size_t pos_cap) {
  Cell c;
  if (!rle_cell(masks, H, W, S, colblocks, c)) return;
  const u64 b = base[blockIdx.y];
  uint32_t off[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) off[k] = c.x0 + k < W ? segoff[c.cell + k] : 0;
  u64 prev = rle_prev(c, H, W);
  const uint8_t* row = c.m + (size_t)c.y0 * W;
  const bool full = c.x0 <= (long long)W - 8;
  const uint32_t p0 = (uint32_t)(c.x0 * H + c.y0);       // position of (x0, y0); H * W < 2^31
  // eight rows per trip, their loads issued before any of them is looked at (a change's store does not wait in between)
  for (int y = 0; y < c.ny; y += 8) {
    u64 cur[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint8_t* r = row + (size_t)min(y + j, c.ny - 1) * W;      // (past the cell: its last row again, not used)
      if (full) {
        u64 v;
        memcpy(&v, r + c.x0, 8);
        cur[j] = norm8(v);
      } else {
        cur[j] = load8(r, c.x0, W);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (y + j >= c.ny) break;
      const u64 diff = cur[j] ^ prev;
      prev = cur[j];
      if (diff) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if ((diff >> (8 * k)) & 1) {
            const u64 at = b + off[k]++;
            if (at < pos_cap) pos[at] = p0 + (uint32_t)k * (uint32_t)H + (uint32_t)(y + j);
          }
      }
    }
  }
}

// the bytes of one value of rleToString, first byte lowest (at most 7 for a 32-bit count); len = how many
__device__ __forceinline__ u64 rle_emit(long long x, int& len) {
  u64 packed = 0;
  bool more;
  len = 0;
  do {
    int ch = (int)(x & 0x1f);
    x >>= 5;
    more = (ch & 0x10) ? x != -1 : x != 0;
    if (more) ch |= 0x20;
    packed |= (u64)(ch + 48) << (8 * len++);
  } while (more && len < 8);
  return packed;
}

// grid n.  Detection d's string goes to str + 7 * (base[d] + d), the room of its T + 1 counts at 7 bytes each.
__global__ __launch_bounds__(RLE_NT) void rle_string_kernel(const uint32_t* __restrict__ pos, const u64* __restrict__ base,
                                                            const uint32_t* __restrict__ totals, size_t pos_cap,
                                                            uint32_t area, uint8_t* __restrict__ str, size_t str_cap,
                                                            u64* __restrict__ lens) {
  __shared__ u64 sm[RLE_WAVES];
  const int d = blockIdx.x;
  const long long T = totals[d];
  const u64 b = base[d];
  const uint32_t* P = pos + b;
  const u64 slot = 7 * (b + (u64)d);
  auto pos_at = [&](long long i) -> uint32_t { return b + (u64)i < pos_cap ? P[i] : 0u; };
  auto count_at = [&](long long i) -> uint32_t {         // 0 <= i <= T
    const uint32_t lo = i == 0 ? 0u : pos_at(i - 1), hi = i == T ? area : pos_at(i);
    return hi - lo;
  };
  u64 carry = 0;
  for (long long i0 = 0; i0 <= T; i0 += RLE_NT * RLE_STR_ITEMS) {
    const long long i = i0 + threadIdx.x * RLE_STR_ITEMS;
    u64 bytes[RLE_STR_ITEMS];
    int len[RLE_STR_ITEMS];
    u64 mine = 0;
#pragma unroll
    for (int j = 0; j < RLE_STR_ITEMS; ++j) {
      len[j] = 0;
      bytes[j] = 0;
      if (i + j <= T) {
        long long x = count_at(i + j);
        if (i + j > 2) x -= count_at(i + j - 2);
        bytes[j] = rle_emit(x, len[j]);
      }
      mine += len[j];
    }
    u64 total;
    u64 at = slot + carry + block_excl_scan<u64>(mine, total, sm);
#pragma unroll
    for (int j = 0; j < RLE_STR_ITEMS; ++j)
      for (int k = 0; k < len[j]; ++k, ++at)
        if (at < str_cap) str[at] = (uint8_t)(bytes[j] >> (8 * k));
    carry += total;
  }
  if (threadIdx.x == 0) lens[d] = carry;
}

// the sizes both entry points share; false when there is nothing to launch
struct RleGeom {
  int S, colblocks;
  size_t cells;          // n * S * W
  unsigned grid_x;
};
bool rle_geom(int n, int H, int W, RleGeom& g) {
  if (n <= 0 || H <= 0 || W <= 0) return false;
  g.S = (int)(((long long)H + RLE_ROWS - 1) / RLE_ROWS);
  g.colblocks = (int)(((long long)W + RLE_WG_COLS - 1) / RLE_WG_COLS);
  g.cells = (size_t)n * g.S * W;
  g.grid_x = (unsigned)((long long)g.colblocks * ((g.S + RLE_WAVES - 1) / RLE_WAVES));   // < H * W / 2^17 + H / 256 + W / 512 + 2
  return true;
}

}  // namespace

extern "C" int as_rle_tile(int* rows_per_segment, int* cols_per_workgroup) {
  AS_REQUIRE(rows_per_segment && cols_per_workgroup, AS_E_BADARG, "as_rle_tile: null pointer");
  *rows_per_segment = RLE_ROWS;
  *cols_per_workgroup = RLE_WG_COLS;
  return AS_OK;
}

extern "C" size_t as_rle_workspace_bytes(int n, int H, int W) {
  RleGeom g;
  if (!rle_geom(n, H, W, g)) return 0;
  return 8 * ((size_t)n + 1) + 5 * g.cells;            // bases (8 bytes each), cell offsets (4), cell counts (1)
}

#define RLE_COMMON_CHECKS(what)                                                                                             \
  AS_REQUIRE(n >= 0 && H >= 0 && W >= 0, AS_E_BADARG, what ": negative size");                                              \
  if (n == 0 || H == 0 || W == 0) return AS_OK;                                                                             \
  AS_REQUIRE(masks && totals && workspace, AS_E_BADARG, what ": null pointer");                                             \
  AS_REQUIRE((unsigned long long)H * (unsigned long long)W <= 0x7fffffffull && n <= 65535, AS_E_UNSUPPORTED,                \
             what ": %d masks of %d x %d (at most 65535 masks of 2^31 - 1 pixels)", n, H, W);                               \
  AS_REQUIRE(workspace_bytes >= as_rle_workspace_bytes(n, H, W), AS_E_WORKSPACE, what ": workspace of %zu bytes, %zu needed", \
             workspace_bytes, as_rle_workspace_bytes(n, H, W));                                                             \
  AS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(totals) & 3) == 0,          \
             AS_E_BADARG, what ": workspace not 8-byte / totals not 4-byte aligned")

extern "C" int as_rle_count(const void* masks, int n, int H, int W, uint32_t* totals, void* workspace, size_t workspace_bytes,
                            as_stream_t stream) {
  RLE_COMMON_CHECKS("as_rle_count");
  RleGeom g;
  rle_geom(n, H, W, g);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* segoff = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(workspace) + 8 * ((size_t)n + 1));
  uint8_t* cnt = reinterpret_cast<uint8_t*>(segoff + g.cells);
  hipLaunchKernelGGL(rle_count_kernel, dim3(g.grid_x, n), dim3(RLE_NT), 0, s, static_cast<const uint8_t*>(masks), H, W, g.S,
                     g.colblocks, cnt);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(n), dim3(RLE_NT), 0, s, cnt, segoff, totals, g.S, W);
  AS_CHECK_LAUNCH("rle_count");
  return AS_OK;
}

extern "C" int as_rle_encode(const void* masks, int n, int H, int W, const uint32_t* totals, void* workspace,
                             size_t workspace_bytes, uint32_t* pos, size_t pos_capacity, void* str, size_t str_capacity,
                             unsigned long long* lens, as_stream_t stream) {
  RLE_COMMON_CHECKS("as_rle_encode");
  AS_REQUIRE(str && lens && (pos || pos_capacity == 0), AS_E_BADARG, "as_rle_encode: null pointer");
  AS_REQUIRE((reinterpret_cast<uintptr_t>(pos) & 3) == 0 && (reinterpret_cast<uintptr_t>(lens) & 7) == 0, AS_E_BADARG,
             "as_rle_encode: pos not 4-byte / lens not 8-byte aligned");
  RleGeom g;
  rle_geom(n, H, W, g);
  hipStream_t s = (hipStream_t)stream;
  u64* base = static_cast<u64*>(workspace);
  const uint32_t* segoff = reinterpret_cast<const uint32_t*>(static_cast<uint8_t*>(workspace) + 8 * ((size_t)n + 1));
  hipLaunchKernelGGL(rle_base_kernel, dim3(1), dim3(RLE_NT), 0, s, totals, n, base);
  if (pos_capacity > 0)
    hipLaunchKernelGGL(rle_fill_kernel, dim3(g.grid_x, n), dim3(RLE_NT), 0, s, static_cast<const uint8_t*>(masks), H, W, g.S,
                       g.colblocks, segoff, base, pos, pos_capacity);
  hipLaunchKernelGGL(rle_string_kernel, dim3(n), dim3(RLE_NT), 0, s, pos, base, totals, pos_capacity, (uint32_t)((size_t)H * W),
                     static_cast<uint8_t*>(str), str_capacity, lens);
  AS_CHECK_LAUNCH("rle_encode");
  return AS_OK;
}
