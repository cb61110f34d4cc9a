// The conv stack's device templates (implicit-GEMM conv layer on v_mfma_f32_16x16x4_f32, BatchNorm + ReLU over the LDS image,
// the LDS region of a frame), shared by the fp32 forward (deepqn.hip) and the float16 forward (dqn16.hip).  The float16
// forward instantiates them with H16 = true: the same fp32 chains with the float16 contract's three rounding points
// (DESIGN.md 6a "Float16 DeepQN"); H16 = false (the default) is the fp32 code, unchanged.
#pragma once
#include "dqn_common.hip.h"
#include "fc16_layout.hip.h"
#include <type_traits>

namespace coevo {

#ifndef DQ_LUT
#define DQ_LUT 0   // 1: /255 through a 256-entry LDS table instead of u8_over_255 (measured equal at 3 workgroups per CU)
#endif
#ifndef DQ_WPE
#define DQ_WPE 6   // waves per SIMD the register budget is set for: 3 workgroups x 8 waves / 4 SIMDs
#endif
#ifndef DQ_QU1
#define DQ_QU1 4
#endif
#ifndef DQ_QU2
#define DQ_QU2 4
#endif
#ifndef DQ_QU3
#define DQ_QU3 4
#endif

// ---------------------------------------------------------------------------------------------------------------
// One conv layer of one frame as an implicit GEMM on v_mfma_f32_16x16x4_f32 (bit-identical to the sequential-k fmaf chain
// from the bias: tools/mfma16_chain_probe.hip; taps in the canonical (ci, ky, kx) order).  M = output positions in tiles
// of 16, N = output channels in pairs of 16-wide tiles, K = taps, four per instruction.  A unit = (position tile, channel
// tile pair): one LDS gather per lane feeds two MFMAs.  Unit u = w + 8 i belongs to wave w (8 waves, two per SIMD: one
// wave's gathers hide behind the other's MFMAs), so all units of a wave share their channel pair and the pair's weight
// operands are loaded once per k-step pair (a chunk of QU k-steps ahead, from L2: the 16 frames of a task and every task
// of the same net read the same 0.3 MB).  Tile padding: 400 = 25 x 16 positions (0 %), 81 -> 96 (16 %), 49 -> 64 (23 %); the 32 x 32 tiles
// this replaces padded 400 -> 512, 81 -> 128, 49 -> 64 and left half of the waves idle in conv3.
//   operands of one MFMA: lane (c = l % 16, kk = l / 16): A[position c of the tile][tap 4 q + kk], B[tap 4 q + kk][channel c];
//   accumulator register r of lane (c, g = l / 16): position 4 g + r of the tile, channel c.
// The raw sums go to LDS as out[channel][position] (odd pitch); BatchNorm + ReLU then runs over them channel by channel.
typedef float f32x4_acc __attribute__((ext_vector_type(4)));

// x / 255.0f for x = 0 .. 255, correctly rounded, without the divide: 1/255 split into a float head and tail,
// fma(x, head, x * tail) equals the IEEE quotient for all 256 inputs (tests/test_host_logic_cpu.py checks the identity
// in numpy; an LDS table of the quotients cost a dependent, bank-conflicted read per gathered tap)
__device__ __forceinline__ float u8_over_255(unsigned b)
{
    constexpr float HEAD = (float)(1.0 / 255.0), TAIL = (float)(1.0 / 255.0 - (double)HEAD);
    const float x = (float)b;
    return __builtin_fmaf(x, HEAD, x * TAIL);
}

// Addressing is organised per chunk of QU k-steps (4 QU taps) so that the MFMA loop issues almost no address arithmetic
// (SQ counters of the first 16x16x4 version: 4 VALU instructions per MFMA - 64-bit weight addresses, tap decoding - kept
// the matrix pipe at 46 %): within a chunk the tap of k-step j, lane group kk is
//   conv1 (8 x 8 window, t = 4 q + kk):  ci = q0 / 16, ky = (q0 / 2) % 8 + j / 2, kx = kk + 4 (j % 2)
//   conv2 (4 x 4):                        ci = q0 / 4 + j / 4, ky = j % 4, kx = kk
// i.e. one per-lane chunk base + a compile-time offset per j (an instruction immediate); conv3's 3 x 3 window repeats every
// nine k-steps instead: nine per-lane addresses + an immediate (Conv16::run).
template <int KS, int HIN, bool U8IN, int IN_PITCH, int CT>
struct TapAddr {
    // offset of tap (chunk q0, step j, lane group kk) = chunk_base(q0, kk) + rel(j)
    __device__ static __forceinline__ int chunk_base(int q0, int kk, int cin)
    {
        if constexpr (KS == 8) {
            const int ci = q0 >> 4, ky0 = (q0 >> 1) & 7;
            return U8IN ? (ky0 * HIN + kk) * (CT ? CT : cin) + ci : ci * IN_PITCH + ky0 * HIN + kk;
        } else {
            return (q0 >> 2) * IN_PITCH + kk;
        }
    }
    __device__ static __forceinline__ int rel(int j, int cin)
    {
        if constexpr (KS == 8) return U8IN ? ((j >> 1) * HIN + 4 * (j & 1)) * (CT ? CT : cin) : (j >> 1) * HIN + 4 * (j & 1);
        else return (j >> 2) * IN_PITCH + (j & 3) * HIN;
    }
};

// H16: the float16 forward - the /255 quotient and the layer's sums are rounded once to fp16 (f16r), everything between is
// the same fp32 chain
template <int KS, int STRIDE, int HIN, int HOUT, int COUT, bool U8IN, int IN_PITCH, int OUT_PITCH, int CT, int QU, bool OVER,
          bool H16 = false>
struct Conv16 {
    static constexpr int NPOS = HOUT * HOUT, NM = (NPOS + 15) / 16, NP = COUT / 32, NUNITS = NM * NP;
    // SPLIT (conv1: 25 units on 8 waves): every wave takes three whole units and the 25th is halved between waves 0 and 1
    // (they sit on different SIMDs), one channel tile each: 7 MFMAs per k-step on the critical waves instead of 8
    static constexpr bool SPLIT = (NP == 1) && (NUNITS % 8 == 1);
    static constexpr int NFULL = NUNITS / 8, REM = SPLIT ? 0 : NUNITS % 8;   // waves w < REM carry NFULL + 1 units
    static_assert(8 % NP == 0, "all units of a wave share their channel pair");
    using Tap = TapAddr<KS, HIN, U8IN, IN_PITCH, CT>;

    // NU whole units (+ the half unit when XL) of wave w, as straight-line code: the unit count is a template argument so
    // that the k-loop has no branches and the scheduler can move a k-step's gathers above the previous step's MFMAs
    // The units are given by the caller: channel pair np (all units of a wave share it), position tile mt[i] of unit i,
    // xh = which channel tile of the last position tile the half unit takes (XL).  in_shift: elements by which `in_lds`
    // starts inside the layer's input image (a kernel that stages only the rows its tile needs).
    template <int NU, bool XL>
    static __device__ __forceinline__ void run(const void *in_lds, const float *lut, int cin, int taps, const float *wt,
                                               const float *bias, float *out, int l, int np,
                                               const int (&mt)[NU > 0 ? NU : 1], int xh, int in_shift)
    {
        const int c = l & 15, kk = l >> 4;
        constexpr int NA = NU > 0 ? NU : 1;
        f32x4_acc acc[NA][2], accx;
        int base[NA], xbase = 0;
        auto tile_base = [&](int m) {
            int p = 16 * m + c;
            if (p >= NPOS) p = 0;   // padded rows read position 0; their results are never stored
            const int oy = p / HOUT, ox = p % HOUT;
            return (U8IN ? ((oy * STRIDE) * HIN + ox * STRIDE) * (CT ? CT : cin) : (oy * STRIDE) * HIN + ox * STRIDE) - in_shift;
        };
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            base[i] = tile_base(mt[i]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float bb = bias[32 * np + 16 * h + c];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][h][r] = bb;
                // pin the splat in a real register tuple: hipcc 7.2 otherwise kept only element 0 of some accumulators
                // live up to the first MFMA and reused elements 1..3 for the loop's address / operand temporaries
                // (seen in the ISA of the three-unit + half-unit instantiation; tests/test_deepqn_gpu.py caught it)
                asm volatile("" : "+v"(acc[i][h]));
            }
        }
        if constexpr (XL) {
            xbase = tile_base(NM - 1);
            const float bb = bias[16 * xh + c];
#pragma unroll
            for (int r = 0; r < 4; ++r) accx[r] = bb;
            asm volatile("" : "+v"(accx));
        }
        // QU = k-steps per chunk: their weight operands are requested together, one chunk AHEAD of the MFMAs that use them
        // (an L2 round trip per chunk would otherwise be exposed: conv2 / conv3 have only one or two units per wave to hide
        // it behind).  This lane's B operands: one float4 per k-step pair (layout: dqn_common.hip.h dqn_conv_slab_to_flat)
        // (buffer loads: wave-uniform descriptor + the chunk's byte offset in an SGPR + the lane's constant 32-bit offset - as
        // global loads every chunk cost a 64-bit vector add, and vector instructions are taken from the matrix pipe's time)
        typedef unsigned u32x4_b __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float *>(wt) + np * 256, 0, 0x7fffffff, 0x00020000);
        float bvA[QU][2], bvB[QU][2];
        int cbA = 0, cbB = 0;    // chunk bases (conv1 / conv2)
        // conv3 (3 x 3 window): k-step q = 9 m + s, lane group kk holds tap t = 36 m + 4 s + kk, i.e. input channel
        // 4 m + (4 s + kk) / 9 and window cell (4 s + kk) % 9: nine per-lane addresses per unit (s = 0 .. 8) + a compile-time
        // 4 m channel pitches (an instruction immediate; the k loop is unrolled) - no vector instruction per gather.  (A
        // 16-bit offset table in LDS cost a table read and a shift-add per gather: half a vector instruction per MFMA.)
        int a9[KS == 3 ? NA : 1][9];
        if constexpr (KS == 3) {
#pragma unroll
            for (int sft = 0; sft < 9; ++sft) {
                const int t = 4 * sft + kk, cell = t % 9;
#pragma unroll
                for (int i = 0; i < NA; ++i) a9[i][sft] = base[i] + (t / 9) * IN_PITCH + (cell / 3) * HIN + cell % 3;
            }
        }
        auto issue = [&](float (&bv)[QU][2], int &cb, int q0) {
#pragma unroll
            for (int jp = 0; jp < QU / 2; ++jp) {
                const u32x4_b v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, 16 * l + jp * (NP * 1024), (q0 >> 1) * (NP * 1024), 0);
                bv[2 * jp][0] = __uint_as_float(v[0]);
                bv[2 * jp][1] = __uint_as_float(v[1]);
                bv[2 * jp + 1][0] = __uint_as_float(v[2]);
                bv[2 * jp + 1][1] = __uint_as_float(v[3]);
            }
            if constexpr (KS != 3) cb = Tap::chunk_base(q0, kk, cin);
        };
        auto consume = [&](const float (&bv)[QU][2], int cb, int qc) {   // qc: the chunk's first k-step (conv3 only)
#pragma unroll
            for (int j = 0; j < QU; ++j) {
                auto gather = [&](int b0, int i) {
                    int off;
                    if constexpr (KS == 3) off = a9[i][(qc + j) % 9] + ((qc + j) / 9) * (4 * IN_PITCH);
                    else off = b0 + cb + Tap::rel(j, cin);
                    if constexpr (U8IN) {
                        const float q = DQ_LUT ? lut[static_cast<const unsigned char *>(in_lds)[off]]
                                               : u8_over_255(static_cast<const unsigned char *>(in_lds)[off]);
                        if constexpr (H16) return f16r_after_fma(q);   // (u8_over_255 ends in an fmaf)
                        else return q;
                    } else return static_cast<const float *>(in_lds)[off];
                };
#pragma unroll
                for (int i = 0; i < NU; ++i) {
                    const float av = gather(base[i], i);
                    acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j][0], acc[i][0], 0, 0, 0);
                    acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j][1], acc[i][1], 0, 0, 0);
                }
                if constexpr (XL) {
                    const float av = gather(xbase, NU);
                    accx = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xh ? bv[j][1] : bv[j][0], accx, 0, 0, 0);
                }
            }
        };
        issue(bvA, cbA, 0);
        if constexpr (KS == 3) {
            constexpr int NQ = 144;   // 64 input channels x 9 cells / 4: fully unrolled (a9's index must be a constant)
            static_assert(!XL && NQ % QU == 0, "conv3: whole units, whole chunks");
#pragma unroll
            for (int q0 = 0; q0 < NQ; q0 += 2 * QU) {
                if (q0 + QU < NQ) issue(bvB, cbB, q0 + QU);
                consume(bvA, cbA, q0);
                if (q0 + QU >= NQ) break;
                if (q0 + 2 * QU < NQ) issue(bvA, cbA, q0 + 2 * QU);
                consume(bvB, cbB, q0 + QU);
            }
        } else {
            const int nq = taps / 4;   // a multiple of QU (C * 16, 128)
            for (int q0 = 0; q0 < nq; q0 += 2 * QU) {
                if (q0 + QU < nq) issue(bvB, cbB, q0 + QU);
                consume(bvA, cbA, 0);
                if (q0 + QU >= nq) break;
                if (q0 + 2 * QU < nq) issue(bvA, cbA, q0 + 2 * QU);
                consume(bvB, cbB, 0);
            }
        }
        if constexpr (OVER) __syncthreads();   // the output overwrites the input: every wave has gathered its last tap
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const int m = mt[i];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int p = 16 * m + 4 * kk + r;
                    if (p < NPOS) out[(32 * np + 16 * h + c) * OUT_PITCH + p] = H16 ? f16r(acc[i][h][r]) : acc[i][h][r];
                }
        }
        if constexpr (XL) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = 16 * (NM - 1) + 4 * kk + r;
                if (p < NPOS) out[(16 * xh + c) * OUT_PITCH + p] = H16 ? f16r(accx[r]) : accx[r];
            }
        }
    }
};

// The whole layer on the eight waves of a frame's workgroup: unit u = w + 8 i belongs to wave w.  w must be wave-uniform in
// an SGPR (readfirstlane): the dispatch below is a scalar branch (every wave runs exactly one instantiation, so the barrier
// inside is reached once by all of them)
template <int KS, int STRIDE, int HIN, int HOUT, int COUT, bool U8IN, int IN_PITCH, int OUT_PITCH, int CT, int QU, bool OVER,
          bool H16 = false>
__device__ __forceinline__ void conv16_mfma(const void *in_lds, const float *lut, int cin, int taps, const float *wt,
                                            const float *bias, float *out, int w, int l)
{
    using K = Conv16<KS, STRIDE, HIN, HOUT, COUT, U8IN, IN_PITCH, OUT_PITCH, CT, QU, OVER, H16>;
    // every wave must enter run<> exactly once: the barrier of an OVER layer sits inside it
    static_assert(K::SPLIT || K::REM == 0 || K::NFULL > 0, "a wave without units would skip run<>'s barrier");
    const int np = w % K::NP;
    auto call = [&](auto nu, auto xl) {
        constexpr int NU = decltype(nu)::value;
        int mt[NU > 0 ? NU : 1];
#pragma unroll
        for (int i = 0; i < (NU > 0 ? NU : 1); ++i) mt[i] = (w + 8 * i) / K::NP;
        K::template run<NU, decltype(xl)::value>(in_lds, lut, cin, taps, wt, bias, out, l, np, mt, w & 1, 0);
    };
    using std::integral_constant;
    if constexpr (K::SPLIT) {
        if (w < 2) call(integral_constant<int, K::NFULL>{}, integral_constant<bool, true>{});
        else call(integral_constant<int, K::NFULL>{}, integral_constant<bool, false>{});
    } else if constexpr (K::REM == 0) {
        call(integral_constant<int, K::NFULL>{}, integral_constant<bool, false>{});
    } else {
        if (w < K::REM) call(integral_constant<int, K::NFULL + 1>{}, integral_constant<bool, false>{});
        else call(integral_constant<int, K::NFULL>{}, integral_constant<bool, false>{});
    }
}

// BatchNorm in training mode at batch 1 (per-sample, per-channel statistics over the NPOS positions) + ReLU, in place on
// x[channel][position] in LDS.  mean = S / N, var = S2 / N (biased), rstd = 1 / sqrtf(var + 1e-5f),
// y = fmaf(d * rstd, gamma, beta).  S = the canonical sum of a channel image (oracle/coevo_oracle.c reduce_strided64): lane l
// adds its positions l, l + 64, l + 128, ... left to right (pad = 0), then the canonical 64-lane tree over the lane sums.
// A wave owns COUT / 8 channels: their lane sums are plain vector adds and ALL the trees of a pass are ONE packed butterfly
// (coevo_common.hip.h: lane k then holds channel k's total); the IEEE divides and the square root run once per pass,
// lane-parallel, and each channel's mean / rstd comes back by v_readlane.  (f32 MFMA and VALU instructions share one
// issue resource - tools/mfma_rate_probe.hip - so every vector instruction of this pass is taken from the other
// workgroups' matrix time.  The first form summed 64-wide blocks by a tree each and chained the block sums: 7 trees per
// channel of conv1's image instead of one, 550 instead of ~250 vector instructions per wave for that pass.)
// H16: the normalised value is rounded once to fp16 before the ReLU (the statistics stay the fp32 rule on the fp16 sums)
template <int NPOS, int PITCH, int COUT, bool H16 = false>
__device__ __forceinline__ void bn_relu_rows(float *x, const float *gamma, const float *beta, int w, int l)
{
    constexpr int NB = (NPOS + 63) / 64, CPW = COUT / 8;
    static_assert(CPW >= 1 && CPW <= 16, "one packed butterfly per pass");
    float v[CPW][NB], s1[CPW], s2[CPW];
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
#pragma unroll
        for (int b = 0; b < NB; ++b) v[k][b] = (64 * b + l < NPOS) ? x[(w + 8 * k) * PITCH + 64 * b + l] : 0.0f;
        s1[k] = v[k][0];
#pragma unroll
        for (int b = 1; b < NB; ++b) s1[k] = s1[k] + v[k][b];
    }
    const float meanv = packed_totals<CPW>(s1, l) / (float)NPOS;   // lane k: channel k's mean
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
        const float mean = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(meanv), k));
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            v[k][b] = v[k][b] - mean;
            const float sq = (64 * b + l < NPOS) ? v[k][b] * v[k][b] : 0.0f;
            s2[k] = (b == 0) ? sq : s2[k] + sq;
        }
    }
    const float varv = packed_totals<CPW>(s2, l) / (float)NPOS;
    const float rstdv = 1.0f / __builtin_sqrtf(varv + LN_EPS);
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
        const int ch = w + 8 * k;
        const float rstd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rstdv), k));
        const float ga = gamma[ch], be = beta[ch];
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (64 * b + l < NPOS) {
                float y = __builtin_fmaf(v[k][b] * rstd, ga, be);
                if constexpr (H16) y = f16r_after_fma(y);
                x[ch * PITCH + 64 * b + l] = relu_keep_nan(y);
            }
    }
}

constexpr int DQ_P1 = 401, DQ_P2 = 81, DQ_P3 = 49;   // channel pitches of the activation images (odd: conflict-free columns)

// One region serves every layer: the frame, then conv1's output written OVER it (conv1 keeps its sums in registers until
// every wave has read its last tap: one extra barrier), conv2's output over that the same way, conv3's next to conv2's.
// 52.5 KB instead of 80.6 KB: three workgroups (24 waves) per CU - while one frame is in a barrier, a BatchNorm pass or its
// staging, two others feed the matrix pipe - and six-channel frames fit the same footprint.
template <int CMAX>
struct DqnSmem {
    float lut[DQ_LUT ? 256 : 1];                   // x / 255.0f for x = 0 .. 255
    union {
        unsigned char frame[84 * 84 * CMAX + 16];  // the uint8 HWC frame (dead after conv1's last gather)
        float a1[32 * DQ_P1];                      // conv1 activations (dead after conv2's last gather)
        struct {
            float a2[64 * DQ_P2];                  // conv2 activations
            float a3[64 * DQ_P3];                  // conv3 activations = the flattened CHW row
        };
    };
};
static_assert(sizeof(DqnSmem<6>) * 3 <= 160 * 1024, "three workgroups per CU");

}  // namespace coevo
