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

// half h of the fc1 block -> fc1.w flat index out * 3136 + k
__host__ __device__ inline int64_t dqn16_fc1_half_to_flat(int64_t h)
{
    const int64_t e = h & 7, l = (h >> 3) & 63, o = (h >> 9) % DQ16_OCTETS, ob = (h >> 9) / DQ16_OCTETS;
    return (ob * 64 + l) * DQ_FC1_IN + 8 * o + e;
}

// word s (outside the fc1 block) of the fp16 slab -> canonical flat index, -1 for the stride's padding
__host__ __device__ inline int64_t dqn16_word_to_flat(int64_t s, int C, int n)
{
    const DqnLayout L16 = dqn16_layout(C, n), L32 = dqn_layout(C, n);
    if (s >= L16.total) return -1;
    return dqn_slab_to_flat(s < L16.wf ? s : s - L16.bf + L32.bf, C, n, 0);
}

// a task the float16 forward cannot serve: the 16-byte fc1 pieces need net_off at a multiple of 4 words
__device__ __forceinline__ bool dqn16_bad_task(const coevo_dqn_task &t)
{
    return t.n_rows < 1 || t.n_rows > COEVO_DQN_MAX_ROWS || (t.net_off & 3) != 0;
}

}  // namespace coevo
