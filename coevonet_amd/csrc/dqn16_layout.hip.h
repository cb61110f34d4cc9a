// The fp16 slab of one DeepQN (args.precision == "float16", Atari/deepqn.py:12-37), shared by the pack / unpack kernels and
// the float16 forward (dqn16.hip).  The layout is ABI (include/coevo.h, coevo_dqn16_*).
#pragma once
#include "dqn_common.hip.h"

namespace coevo {

// ---- fp16 slab layout of one net, in 32-bit words (the unit of coevo_dqn_task.net_off) ------------------------------
// Every section of the fp32 slab (dqn_common.hip.h dqn_layout) in the same order and, but for fc1, the same form:
//   w1 b1/g1/be1 w2 b2/g2/be2 w3 b3/g3/be3   fp32 WORDS that hold fp16 values: the conv weights in the lane order of
//                                            conv16_mfma (dqn_conv_slab_to_flat; 0.3 MB per net, served from L2), the
//                                            biases and the BatchNorm affine (half in the reference: vbn*.to(float16))
//   wfh [8][392][64][8] half                 fc1.weight, 95 % of a net, as 2-byte values: the 16-byte piece of lane l in
//                                            (output block ob, k-octet o) holds fc1.w[64 ob + l][8 o .. 8 o + 7] - eight
//                                            consecutive k of the lane's own output, one non-temporal load
//   bf [512], wo [n][512], bo [n]            fp32 words that hold fp16 values
// Every section starts at a multiple of 4 words; the stride is padded to a multiple of 64 words (256 bytes).
// C = 4, n = 6: 884 710 words used, against 1 687 526 of the fp32 slab.
constexpr int64_t DQ16_FC1_WORDS = (int64_t)DQ_FC1_OUT * DQ_FC1_IN / 2;
constexpr int DQ16_OCTETS = DQ_FC1_IN / 8;   // 392 k-octets per output

__host__ __device__ inline DqnLayout dqn16_layout(int C, int n)
{
    DqnLayout L = dqn_layout(C, n);   // the sections in front of fc1 are the fp32 slab's
    L.bf = L.wf + DQ16_FC1_WORDS;
    L.wo = L.bf + DQ_FC1_OUT;
    L.bo = L.wo + (int64_t)n * DQ_FC1_OUT;
    L.total = L.bo + n;
    L.stride = (L.total + 63) / 64 * 64;
    return L;
}

// The fc1 block has a second form, a permutation of its halves (the slab's sections, offsets and stride are the same), reached
// through the entry points of include/coevo_ext.h only (coevo_dqn16_*_tiled; dqn16_tiled.hip):
//   wft16 [8][98][4][64][8] half             tiled: the 16-byte piece of lane (c = l % 16, kk = l / 16) in (output block ob,
//                                            super-piece S, column tile T) holds fc1.w[64 ob + 16 T + c][32 S + 4 j + kk], j = 0 .. 7
//                                            - for tile T the B operands of the eight consecutive v_mfma_f32_16x16x4 k-quads
//                                            8 S .. 8 S + 7.  A wave reads 1 KiB contiguously per (S, T) and a (task, ob) wave
//                                            streams 98 x 4 KiB = 401 408 bytes as one run: the streamed form's bytes
constexpr int DQ16_SUPER = DQ_FC1_IN / 32;   // 98 super-pieces (32 k) per output block

// half h of the fc1 block -> fc1.w flat index out * 3136 + k
__host__ __device__ inline int64_t dqn16_fc1_half_to_flat(int64_t h, int tiled = 0)
{
    if (tiled) {
        const int64_t j = h & 7, l = (h >> 3) & 63, T = (h >> 9) & 3, S = (h >> 11) % DQ16_SUPER, ob = (h >> 11) / DQ16_SUPER;
        return (ob * 64 + 16 * T + (l & 15)) * DQ_FC1_IN + 32 * S + 4 * j + (l >> 4);
    }
    const int64_t e = h & 7, l = (h >> 3) & 63, o = (h >> 9) % DQ16_OCTETS, ob = (h >> 9) / DQ16_OCTETS;
    return (ob * 64 + l) * DQ_FC1_IN + 8 * o + e;
}

// ... and back: fc1.w[out][k] -> half of the fc1 block
__host__ __device__ inline int64_t dqn16_fc1_flat_to_half(int64_t out, int64_t k, int tiled)
{
    const int64_t ob = out >> 6, o = out & 63;
    if (tiled) return ((((ob * DQ16_SUPER + (k >> 5)) * 4 + (o >> 4)) * 64 + 16 * (k & 3) + (o & 15)) << 3) + ((k >> 2) & 7);
    return (((ob * DQ16_OCTETS + (k >> 3)) * 64 + o) << 3) + (k & 7);
}

// word s (outside the fc1 block) of the fp16 slab -> canonical flat index, -1 for the stride's padding
__host__ __device__ inline int64_t dqn16_word_to_flat(int64_t s, int C, int n)
{
    const DqnLayout L16 = dqn16_layout(C, n), L32 = dqn_layout(C, n);
    if (s >= L16.total) return -1;
    return dqn_slab_to_flat(s < L16.wf ? s : s - L16.bf + L32.bf, C, n, 0);
}

// pack / unpack of one 32-bit word of one net's stride (thread = word, blockIdx.y = net; fc1_tiled: the form of the slab's fc1
// block).  to_slab: every entry is rounded to fp16 to nearest even (exact for fp16 values; the reference's .to(float16)), the
// padding is zeroed.  Else slab -> flat (fp16 values as fp32).
__device__ __forceinline__ void dqn16_pack_word(float *flat, uint32_t *slab, int C, int n, bool to_slab, int fc1_tiled)
{
    const DqnLayout L = dqn16_layout(C, n);
    const int64_t P = dqn_param_count(C, n);
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= L.stride) return;
    uint32_t *word = slab + (int64_t)blockIdx.y * L.stride + s;
    float *f = flat + (int64_t)blockIdx.y * P;
    if (s >= L.wf && s < L.bf) {
        const int64_t F_wf = 32LL * C * 64 + 32 + 64LL * 512 + 64 + 64LL * 576 + 64, h = 2 * (s - L.wf);
        float *f0 = f + F_wf + dqn16_fc1_half_to_flat(h, fc1_tiled), *f1 = f + F_wf + dqn16_fc1_half_to_flat(h + 1, fc1_tiled);
        _Float16 pair[2];
        if (to_slab) {
            pair[0] = (_Float16)*f0;
            pair[1] = (_Float16)*f1;
            __builtin_memcpy(word, pair, 4);
        } else {
            __builtin_memcpy(pair, word, 4);
            *f0 = (float)pair[0];
            *f1 = (float)pair[1];
        }
        return;
    }
    const int64_t p = dqn16_word_to_flat(s, C, n);
    if (to_slab) *word = (p >= 0) ? __float_as_uint(f16r(f[p])) : 0u;
    else if (p >= 0) f[p] = __uint_as_float(*word);
}

// a task the float16 forward cannot serve: the 16-byte fc1 pieces need net_off at a multiple of 4 words
__device__ __forceinline__ bool dqn16_bad_task(const coevo_dqn_task &t)
{
    return t.n_rows < 1 || t.n_rows > COEVO_DQN_MAX_ROWS || (t.net_off & 3) != 0;
}

// the fc1 launch over a tiled fc1 block (defined in dqn16_tiled.hip; dqn16.hip's forward driver enqueues it between its conv and
// output launches): act -> hid for every task, COEVO_ST_BAD_TASK as dqn16_fc1_kernel reports it
void dqn16_fc1_tiled_launch(const uint32_t *slab, const coevo_dqn_task *tasks, int n_tasks, int C, int n_actions, const float *act,
                            float *hid, int32_t *status, hipStream_t stream);

}  // namespace coevo
