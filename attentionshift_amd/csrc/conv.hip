// as_conv2d_fwd: channels-last implicit-GEMM convolution, stride 1, padding (ksize - 1) / 2, ksize 1 or 3.
// The FPN's laterals (1x1, with the top-down nearest upsample folded into the epilogue) and output convolutions (3x3),
// and the RPN trunk (3x3 + ReLU, then cls | reg as one 1x1).
//
// The GEMM: D[n][m] = sum_k W[n][k] . A[m][k] with m = a pixel of the flattened [B, H, W] index space, n = an output channel
// and k = (tap, ci) tap-major -- the nine taps are nine K segments.  There is no im2col buffer and no padded copy: the A
// tile of a K step is 128 pixel rows x 32 input channels (64 bytes) of ONE tap, and the LDS-DMA's per-lane source offset
// points each row at its own shifted pixel (y + dy, x + dx).  A row whose tap lies outside the image is pointed at its
// centre pixel instead (an address inside the tensor) and the lane that owns that row in the MFMA clears its fragment
// registers before the multiply: such taps contribute exact zeros whatever the input holds.
//
// Pipeline as in gemm.hip's bf16 path: K step 32, a 3-deep LDS ring, two steps in flight under the one consumed, counted
// `s_waitcnt vmcnt(N)` + one raw s_barrier per step, the chunk swizzle lds_swz_row<2> applied on the source address, hidden
// fragment reads completed by lds_wait (lds_asm.h).  The DMA goes through lds_dma16 (saddr form: 32-bit byte offsets from
// the tensor's base; the launcher refuses tensors whose span does not fit).
//
// Two tiles (conv_bn): 128 pixels x 128 channels (four waves of 64 x 64, Cout >= 96) and 128 pixels x 32 channels (four
// waves of 32 x 32: the 16-row RPN heads, small necks).  Every wave issues the same number of DMAs per step (the vmcnt
// counts depend on it): in the narrow tile the W tile has two 1-KiB pieces and waves 2, 3 load them a second time.
//
// Epilogue, straight from the accumulators (a lane owns one pixel and runs of four consecutive channels): fp32 accumulator
// + bias, + float(add[b, sy(y), sx(x), n]) (ATen's nearest index), ReLU, one rounding; 8-byte (bf16) or 16-byte (fp32)
// vector stores.  The result is a pure function of the inputs: no atomics, no split-K, no workgroup waits for another.
#include "lds_asm.h"

namespace {

constexpr int CV_BM = 128, CV_GK = 32, CV_ROWB = 64, CV_NSTAGE = 3, CV_NT = 256;

template <int BN> struct CvTile {
  static constexpr int WN = BN == 128 ? 2 : 1, WM = 4 / WN;      // waves along n / m
  static constexpr int RI = CV_BM / (32 * WM), NJ = BN / (32 * WN);   // 32-row blocks of m / n per wave: 2, 2 or 1, 1
  static constexpr int A_BYTES = CV_BM * CV_ROWB, W_BYTES = BN * CV_ROWB, STAGE = A_BYTES + W_BYTES;
  static constexpr int NAP = 2;                                  // 1-KiB pieces (16 rows) of A per wave per step
  static constexpr int W_PIECES = W_BYTES / 1024;                // 8 or 2
  static constexpr int NWP = W_PIECES >= 4 ? W_PIECES / 4 : 1;   // per wave: 2, or 1 (loaded twice over in the narrow tile)
  static constexpr int LOADS = NAP + NWP;
  static constexpr int LDS = CV_NSTAGE * STAGE;                  // 48 KiB / 30 KiB
};

struct ConvArgs {
  const char* x;            // bf16 [B][H][W][Cin], batch stride xbs elements
  const char* w;            // bf16 [Cout][taps][Cin]
  const float* bias;        // [Cout] or null
  const __bf16* add;        // [B][Ha][Wa][Cout] or null
  void* out;                // [B][H][W][Cout]
  long long xbs;
  float sch, scw;           // (float)Ha / H, (float)Wa / W
  int B, H, W, Cin, Cout, ksize, act, Ha, Wa;
};

template <int BN, typename TO>
__global__ __launch_bounds__(CV_NT, 2) void conv2d_kernel(const ConvArgs a) {
  using CT = CvTile<BN>;
  constexpr int RI = CT::RI, NJ = CT::NJ, WN = CT::WN, NAP = CT::NAP, NWP = CT::NWP, STAGE = CT::STAGE;
  extern __shared__ __attribute__((aligned(16))) char smem[];    // [3 stages][A tile | W tile]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, half = lane >> 5;
  const int H = a.H, W = a.W, HW = a.H * a.W, Cin = a.Cin, Cout = a.Cout;
  const int M = a.B * HW;
  const int taps = a.ksize * a.ksize, pad = (a.ksize - 1) >> 1;
  const int nt_n = (Cout + BN - 1) / BN;
  const int m0 = ((int)blockIdx.x / nt_n) * CV_BM, n0 = ((int)blockIdx.x % nt_n) * BN;
  const int kcpt = Cin / CV_GK;                                  // K steps per tap
  const int nk = taps * kcpt;

  // loader: wave w moves A pieces 2w, 2w + 1 (tile rows 16p .. 16p + 15; lane = row lr, chunk slot lc)
  const int lr = lane >> 2, lc = lane & 3;
  unsigned cenA[NAP];                                            // byte offset of the row's own pixel + its swizzled chunk
  int yA[NAP], xA[NAP];
#pragma unroll
  for (int j = 0; j < NAP; ++j) {
    const int r = (wave * NAP + j) * 16 + lr;
    const int p = min(m0 + r, M - 1);
    const int b = p / HW, hw = p - b * HW;
    yA[j] = hw / W;
    xA[j] = hw - yA[j] * W;
    cenA[j] = (unsigned)(((long long)b * a.xbs + (long long)hw * Cin) * 2) + (unsigned)((lc ^ lds_swz_row<2>(r)) * 16);
  }
  unsigned rowW[NWP];                                            // byte offset of (row n, tap 0, ci 0) + its swizzled chunk
#pragma unroll
  for (int j = 0; j < NWP; ++j) {
    const int piece = (wave * NWP + j) % CT::W_PIECES;
    const int r = piece * 16 + lr;
    rowW[j] = (unsigned)(min(n0 + r, Cout - 1) * taps * Cin * 2) + (unsigned)((lc ^ lds_swz_row<2>(r)) * 16);
  }
  const unsigned smem_base = lds_addr(smem);
  int s_tap = 0, s_kc = 0;                                       // the next step to stage (stage() is called in step order)
  auto stage = [&](int buf) {
    const int dy = s_tap / a.ksize - pad, dx = s_tap % a.ksize - pad;
    const unsigned base = smem_base + buf * STAGE;
#pragma unroll
    for (int j = 0; j < NAP; ++j) {
      const bool in = (unsigned)(yA[j] + dy) < (unsigned)H && (unsigned)(xA[j] + dx) < (unsigned)W;
      const unsigned off = cenA[j] + (in ? (unsigned)((dy * W + dx) * Cin * 2) : 0u) + (unsigned)(s_kc * CV_ROWB);
      lds_dma16(off, a.x, __builtin_amdgcn_readfirstlane(base + (wave * NAP + j) * 1024));
    }
#pragma unroll
    for (int j = 0; j < NWP; ++j) {
      const int piece = (wave * NWP + j) % CT::W_PIECES;
      const unsigned off = rowW[j] + (unsigned)((s_tap * Cin + s_kc * CV_GK) * 2);
      lds_dma16(off, a.w, __builtin_amdgcn_readfirstlane(base + CT::A_BYTES + piece * 1024));
    }
    if (++s_kc == kcpt) {
      s_kc = 0;
      ++s_tap;
    }
  };

  // consumer: this lane's pixel rows (one per 32-row block) and, per row, which taps lie inside the image
  unsigned inside[RI];
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int p = min(m0 + wm * (32 * RI) + i * 32 + li, M - 1);
    const int hw = p % HW, y = hw / W, x = hw - y * W;
    unsigned bits = 0;
    for (int t = 0; t < taps; ++t) {
      const int dy = t / a.ksize - pad, dx = t % a.ksize - pad;
      if ((unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W) bits |= 1u << t;
    }
    inside[i] = bits;
  }

  f32x16 acc[RI][NJ];                                            // D[n][m]: [i: 32-block of m][j: 32-block of n]
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  unsigned offA[2], offW[2];                                     // per-lane fragment addresses of block 0, k16 steps 0 / 1
  {
    const int ra = wm * (32 * RI) + li, rb = wn * (32 * NJ) + li;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int g = ks * 2 + half;
      offA[ks] = smem_base + ra * CV_ROWB + ((g ^ lds_swz_row<2>(ra)) << 4);
      offW[ks] = smem_base + CT::A_BYTES + rb * CV_ROWB + ((g ^ lds_swz_row<2>(rb)) << 4);
    }
  }

  stage(0);
  if (nk > 1) stage(1);
  int c_tap = 0, c_kc = 0;                                       // the step being consumed
  for (int kt0 = 0; kt0 < nk; kt0 += CV_NSTAGE) {
    static_for<CV_NSTAGE>([&](auto slot_c) {
      constexpr int slot = decltype(slot_c)::value;
      const int kt = kt0 + slot;
      if (kt >= nk) return;
      // my pieces of step kt have landed when at most the one newer step is still in flight
      if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CT::LOADS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                              // publishes step kt; everyone is done reading step kt - 1
      if (kt + 2 < nk) stage((slot + 2) % CV_NSTAGE);
      constexpr int NF = RI + NJ;
      u32x4 f[2 * NF];                                           // [ks][A0 .. A(RI-1), W0 .. W(NJ-1)]
      static_for<2>([&](auto ks_c) {
        constexpr int ks = decltype(ks_c)::value;
        static_for<RI>([&](auto i_c) {
          constexpr int i = decltype(i_c)::value;
          lds_read128_i<slot * STAGE + i * 32 * CV_ROWB>(f[ks * NF + i], offA[ks]);
        });
        static_for<NJ>([&](auto j_c) {
          constexpr int j = decltype(j_c)::value;
          lds_read128_i<slot * STAGE + j * 32 * CV_ROWB>(f[ks * NF + RI + j], offW[ks]);
        });
      });
      static_for<2>([&](auto ks_c) {
        constexpr int ks = decltype(ks_c)::value;
        constexpr int LEFT = ks == 0 ? NF : 0;                   // LDS returns in order
        u32x4* const p = &f[ks * NF];
        if constexpr (NF == 4) lds_wait<LEFT>(p[0], p[1], p[2], p[3]);
        else lds_wait<LEFT>(p[0], p[1]);
#pragma unroll
        for (int i = 0; i < RI; ++i) {
          Frag<__bf16> fa;
          const u32x4 zero = {0u, 0u, 0u, 0u};
          const u32x4 av = ((inside[i] >> c_tap) & 1u) ? p[i] : zero;   // a tap outside the image: exact zeros
          fa.v = __builtin_bit_cast(bf16x8, av);
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            Frag<__bf16> fb;
            fb.v = __builtin_bit_cast(bf16x8, p[RI + j]);
            acc[i][j] = mma32(fb, fa, acc[i][j]);
          }
        }
      });
      if (++c_kc == kcpt) {
        c_kc = 0;
        ++c_tap;
      }
    });
  }

  // epilogue: lane = pixel li of block i; registers 4g .. 4g + 3 = channels 8g + 4 half + 0 .. 3 of block j
  TO* const out = reinterpret_cast<TO*>(a.out);
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    const int p = m0 + wm * (32 * RI) + i * 32 + li;
    if (p >= M) continue;
    const __bf16* addp = nullptr;
    if (a.add) {
      const int b = p / HW, hw = p - b * HW, y = hw / W, x = hw - y * W;
      const int sy = min((int)floorf((float)y * a.sch), a.Ha - 1), sx = min((int)floorf((float)x * a.scw), a.Wa - 1);
      addp = a.add + ((size_t)(b * a.Ha + sy) * a.Wa + sx) * Cout;
    }
    TO* const orow = out + (size_t)p * Cout;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * (32 * NJ) + j * 32 + 8 * g + 4 * half;
        if (n >= Cout) continue;                                 // Cout % 16 == 0: a run of four is inside or outside whole
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = acc[i][j][4 * g + t];
        if (a.bias) {
          const float4 bv = *reinterpret_cast<const float4*>(a.bias + n);
          v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
        }
        if (addp) {
          const bf16x4 av = *reinterpret_cast<const bf16x4*>(addp + n);
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] += (float)av[t];
        }
        if (a.act == 1) {
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.0f);
        }
        if constexpr (std::is_same<TO, float>::value) {
          *reinterpret_cast<float4*>(orow + n) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
          bf16x4 ov;
#pragma unroll
          for (int t = 0; t < 4; ++t) ov[t] = (__bf16)v[t];
          *reinterpret_cast<bf16x4*>(orow + n) = ov;
        }
      }
  }
}

template <int BN, typename TO> int launch_conv(const ConvArgs& a, hipStream_t s) {
  const long long M = (long long)a.B * a.H * a.W;
  const long long tiles = ((M + CV_BM - 1) / CV_BM) * ((a.Cout + BN - 1) / BN);
  hipLaunchKernelGGL((conv2d_kernel<BN, TO>), dim3((unsigned)tiles), dim3(CV_NT), CvTile<BN>::LDS, s, a);
  AS_CHECK_LAUNCH("as_conv2d_fwd");
  return AS_OK;
}

int conv_bn(int Cout) { return Cout >= 96 ? 128 : 32; }

}  // namespace

extern "C" int as_conv2d_tile_n(int Cout) { return Cout > 0 ? conv_bn(Cout) : 0; }

extern "C" int as_conv2d_fwd(const void* x, long long x_batch_stride, const void* w, const float* bias, const void* add, int Ha,
                             int Wa, int B, int H, int W, int Cin, int Cout, int ksize, int act, int out_dtype, void* out,
                             as_stream_t stream) {
  AS_REQUIRE(x && w && out, AS_E_BADARG, "as_conv2d_fwd: null pointer (x, w or out)");
  AS_REQUIRE(ksize == 1 || ksize == 3, AS_E_BADARG, "as_conv2d_fwd: ksize = %d (1 or 3)", ksize);
  AS_REQUIRE(B > 0 && H > 0 && W > 0, AS_E_BADARG, "as_conv2d_fwd: empty problem B = %d, H = %d, W = %d", B, H, W);
  AS_REQUIRE(Cin > 0 && Cin % 32 == 0, AS_E_BADARG, "as_conv2d_fwd: Cin = %d (a positive multiple of 32)", Cin);
  AS_REQUIRE(Cout > 0 && Cout % 16 == 0, AS_E_BADARG, "as_conv2d_fwd: Cout = %d (a positive multiple of 16)", Cout);
  AS_REQUIRE(act == 0 || act == 1, AS_E_BADARG, "as_conv2d_fwd: act = %d (0 none, 1 relu)", act);
  AS_REQUIRE(out_dtype == AS_F32 || out_dtype == AS_BF16, AS_E_BADARG, "as_conv2d_fwd: out_dtype = %d", out_dtype);
  AS_REQUIRE(x_batch_stride >= (long long)H * W * Cin && x_batch_stride % 8 == 0, AS_E_BADARG,
             "as_conv2d_fwd: batch stride %lld (at least H W Cin = %lld elements, a multiple of 8)", x_batch_stride,
             (long long)H * W * Cin);
  AS_REQUIRE(!add || (Ha > 0 && Wa > 0 && Ha <= H && Wa <= W), AS_E_BADARG,
             "as_conv2d_fwd: add of %d x %d onto %d x %d (1 .. the output's size)", Ha, Wa, H, W);
  AS_REQUIRE(((uintptr_t)x | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)add) % 16 == 0, AS_E_BADARG,
             "as_conv2d_fwd: pointers must be 16-byte aligned");
  // the LDS-DMA takes 32-bit byte offsets from the tensor's base; the pixel index is an int
  const long long span = ((long long)(B - 1) * x_batch_stride + (long long)H * W * Cin) * 2;
  AS_REQUIRE(span < (1ll << 31) && (long long)Cout * ksize * ksize * Cin * 2 < (1ll << 31) && (long long)B * H * W < (1ll << 30),
             AS_E_UNSUPPORTED, "as_conv2d_fwd: the input spans %lld bytes (below 2^31), B H W = %lld (below 2^30)", span,
             (long long)B * H * W);
  ConvArgs a;
  a.x = reinterpret_cast<const char*>(x);
  a.w = reinterpret_cast<const char*>(w);
  a.bias = bias;
  a.add = reinterpret_cast<const __bf16*>(add);
  a.out = out;
  a.xbs = x_batch_stride;
  a.sch = add ? (float)Ha / (float)H : 1.0f;
  a.scw = add ? (float)Wa / (float)W : 1.0f;
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ksize = ksize; a.act = act;
  a.Ha = add ? Ha : 1; a.Wa = add ? Wa : 1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool f32 = out_dtype == AS_F32;
  if (conv_bn(Cout) == 128) return f32 ? launch_conv<128, float>(a, s) : launch_conv<128, __bf16>(a, s);
  return f32 ? launch_conv<32, float>(a, s) : launch_conv<32, __bf16>(a, s);
}
