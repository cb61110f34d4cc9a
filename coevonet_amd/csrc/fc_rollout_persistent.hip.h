// ---- The PERSISTENT form of the small launch: a whole rollout (n_cycles env-cycles) in ONE launch ---------------------------
// ("device-side env step fused with the forward into a persistent whole-rollout kernel".)  A launch that the small
// kernel serves has no more workgroups than the device has CUs, so all of them are resident at once (<= 256 registers, < 80 KiB
// of LDS: two fit a CU, i.e. even two such launches side by side are resident together) and a workgroup can keep its task for the
// whole rollout: W1t / the LayerNorm(512) affine / W3 stay in LDS, the small parameters in registers, every row's game (fp64
// state + the reward books) in LDS - no state buffer is read or written between the reset and the last cycle.  What the rows of
// a game owe each other per cycle is three small integers: a row posts its action as ONE 32-bit word (cycle + 1) << 8 | action
// (agent-scope atomic store, double buffered by cycle parity: a row can be at most one cycle ahead of the rows it plays with),
// and the rows of cycle c spin on the three words of their game until all carry the tag c (agent-scope atomic loads; bounded: a
// workgroup that waits too long - a third such launch squeezed its partners off the chip - raises COEVO_ST_SYNC_TIMEOUT and
// the abort word, which every waiter also watches, so the grid drains).  The data IS the flag: nothing else crosses between
// workgroups, so no fence and no cache maintenance is needed.
// The arithmetic is fc_policy_body_c<R, MODE_FUSED, FC2_DPP>'s and mpe_fused_observe's, operation for operation; the last cycle
// leaves the state buffer and the plain action words exactly as the per-cycle launches do, for coevo_mpe_final_step.
#pragma once
#include "fc_body_compact.hip.h"

namespace coevo {

template <int R>
struct FcSmemP {
    static constexpr int NG = (R + 3) / 4;
    float par[13 * H1];                      // resident: W1t [D][512], fc1.bias, ln1.weight, ln1.bias
    float h1r[R][H1];                        // fc2's activations, row-major (FC2_DPP)
    float h2[R][260];
    float w3s[NACT][260];                    // resident
    float xs0[4 * NG][COEVO_OBS_STRIDE];
    float red[4][16], red2[4][16];
    float logit[R][COEVO_LOGIT_STRIDE];
    double gs[8][24];                        // per row: its game (MpeGame, 18 doubles) + the books [18..21]
    float p2[3][H2];                         // resident: fc2.bias, ln2.weight, ln2.bias (read where used: registers are short)
    float pb3[8];                            // output.bias
    int rowinfo[8][4];                       // per row: game, env slot, agent-step limit
    int ctl[4];                              // [0]: leave the cycle loop (a wait timed out somewhere)
};

#ifndef COEVO_SYNC_SPINS
#define COEVO_SYNC_SPINS (1 << 21)   // polls of ~0.5-1 us each before a waiting row gives up (seconds, not microseconds)
#endif

struct PersistArgs {
    int n_cycles;
    int32_t *sync;        // [4 + 2 * 3 * n_games]: [0] abort word, tagged actions [parity][game][slot] from [4]; zeroed before the launch
    double *state_alt;    // the second state buffer (buffer 1); a.state is buffer 0 (the reset state)
    int32_t *act_plain;   // actions_by_game [2][n_games][3]: only the last cycle's plain actions are written
    double *rewards;      // [n_games][3] or NULL: each game's owner row closes the books itself (mpe_final_step_kernel's arithmetic)
    coevo_final_pack pack;   // .out != NULL: ... and writes this rank's all-gather record (mpe_final_step_kernel's)
};

__global__ void sync_clear_kernel(int32_t *w, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = 0;
}

// a row's game out of its LDS record gs[0..17], and the fields a world step moves (positions, velocities) back
__device__ __forceinline__ void game_from_lds(const double *gs, MpeGame &s)
{
    s.ax = gs[0]; s.ay = gs[1]; s.bx = gs[2]; s.by = gs[3]; s.cx = gs[4]; s.cy = gs[5];
    s.avx = gs[6]; s.avy = gs[7]; s.bvx = gs[8]; s.bvy = gs[9]; s.cvx = gs[10]; s.cvy = gs[11];
    s.l0x = gs[12]; s.l0y = gs[13]; s.l1x = gs[14]; s.l1y = gs[15]; s.gx = gs[16]; s.gy = gs[17];
}
__device__ __forceinline__ void game_moved_to_lds(double *gs, const MpeGame &s)
{
    gs[0] = s.ax; gs[1] = s.ay; gs[2] = s.bx; gs[3] = s.by; gs[4] = s.cx; gs[5] = s.cy;
    gs[6] = s.avx; gs[7] = s.avy; gs[8] = s.bvx; gs[9] = s.bvy; gs[10] = s.cvx; gs[11] = s.cvy;
}

// Bounded wait until the three tagged action words of a game (tp[0..2]) all carry `tag`; gives up early when somebody raised
// the abort word.  False: timed out, or somebody else did - the caller raises COEVO_ST_SYNC_TIMEOUT and the abort word.
struct TaggedWords { bool ok; int w0, w1, w2; };
__device__ __forceinline__ TaggedWords wait_tagged_actions(const int32_t *tp, const int32_t *abort_word, int tag)
{
    int w0 = 0, w1 = 0, w2 = 0;
    bool ok = false;
    for (int it = 0; it < COEVO_SYNC_SPINS; ++it) {
        w0 = __hip_atomic_load(tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w1 = __hip_atomic_load(tp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w2 = __hip_atomic_load(tp + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = (w0 >> 8) == tag && (w1 >> 8) == tag && (w2 >> 8) == tag;
        if (ok) break;
        // (the abort word is ONE word for everybody - agent-scope loads are served by memory, and a thousand
        // lanes on one line queue up: looked at every 16th poll only)
        if ((it & 15) == 15 && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        __builtin_amdgcn_s_sleep(1);
    }
    return {ok, w0, w1, w2};
}

template <int R>
__global__ __launch_bounds__(256, 2) void fc_rollout_small_kernel(FcArgs a, PersistArgs pa)
{
    __shared__ __attribute__((aligned(16))) FcSmemP<R> sm;
    static_assert(sizeof(FcSmemP<R>) <= 80 * 1024, "two workgroups per CU");
    constexpr int NG = FcSmemP<R>::NG;
    constexpr int US = COEVO_SMALL_U;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const bool heavy = (int)blockIdx.x < a.n_heavy;   // workgroup-uniform
    const coevo_fc_task task = heavy ? a.tasks[blockIdx.x] : a.light_tasks[(int)blockIdx.x - a.n_heavy];
    const int D = task.D, nrows = task.n_rows, row0 = task.row_begin;
    const float *net = a.slab + task.net_off;
    const size_t N = (size_t)a.n_games;
    int st = 0;

    // ---- once: parameters into LDS / registers, every row's game into LDS ---------------------------------------------------
    const int n_pieces = (D + 3) * (H1 / 4);
#pragma unroll
    for (int j = 0; j < 7; ++j)
        if (64 * w + 256 * j < n_pieces)   // wave-uniform
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(net + 4 * (t + 256 * j)),
                                             (__attribute__((address_space(3))) void *)(&sm.par[4 * (64 * w + 256 * j)]),
                                             16, 0, 0);
    {
        const float *W3 = net + fc_off_w3(D);
#pragma unroll
        for (int j = 0; j < 5; ++j) sm.w3s[(t + 256 * j) >> 8][(t + 256 * j) & 255] = W3[t + 256 * j];
    }
    {
        const float *b2p = net + fc_off_b2(D);
        sm.p2[0][t] = b2p[t]; sm.p2[1][t] = b2p[H2 + t]; sm.p2[2][t] = b2p[2 * H2 + t];
        if (t < NACT) sm.pb3[t] = net[fc_off_b3(D) + t];
    }
    const float4 *wps = reinterpret_cast<const float4 *>(net + fc_off_w2(D)) + (size_t)w * 128 * 64 + l;
    float4 sbufA[US], sbufB[US];
    if (w == 0 && l < nrows) {
        const int g = a.row_game[row0 + l];
        sm.rowinfo[l][0] = g;
        sm.rowinfo[l][1] = a.row_slot[row0 + l];
        sm.rowinfo[l][2] = a.game_limit ? a.game_limit[g] : 0x7fffffff;
#pragma unroll
        for (int f = 0; f < 22; ++f) sm.gs[l][f] = a.state[(size_t)f * N + g];
    }
    if (t == 0) sm.ctl[0] = 0;
    int32_t *const tags = pa.sync + 4;

    for (int c = 0; c < pa.n_cycles; ++c) {
        // (an opaque zero in the once-per-cycle global addresses of wave 0: left alone, the compiler computes all of them in
        // front of the loop and spills them across it)
        int zero;
        asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
        // ---- env step + observation: one lane per row (wave 0); cycle c > 0 first waits for the three actions of cycle c - 1 --
        // (the first two buffers of this cycle's fc2 stream are requested by waves 1-3 as soon as they get here - under wave 0's
        // output chain of the previous cycle, its wait and its env step - and by wave 0 behind its env step, whose fp64 state is the
        // kernel's register peak: held across it they spilled)
        auto prefetch = [&]() {
#pragma unroll
            for (int uu = 0; uu < US; ++uu) sbufA[uu] = wps[(size_t)uu * 64];
#pragma unroll
            for (int uu = 0; uu < US; ++uu) sbufB[uu] = wps[(size_t)(US + uu) * 64];
        };
        if (w != 0) {
            prefetch();
        } else {
        if (l < 4 * NG) {
            float o[COEVO_OBS_STRIDE];
#pragma unroll
            for (int k = 0; k < COEVO_OBS_STRIDE; ++k) o[k] = 0.0f;
            if (l < nrows) {
                const int g = sm.rowinfo[l][0], slot = sm.rowinfo[l][1], limit = sm.rowinfo[l][2];
                MpeGame s;
                game_from_lds(sm.gs[l], s);
                if (c > 0) {
                    const int32_t *tp = tags + (size_t)((c - 1) & 1) * 3 * N + 3 * (size_t)(g + zero);
                    const TaggedWords tw = wait_tagged_actions(tp, pa.sync, c);
                    const int w0 = tw.w0, w1 = tw.w1, w2 = tw.w2;
                    if (!tw.ok) {   // timed out, or somebody else did: everybody leaves
                        st |= COEVO_ST_SYNC_TIMEOUT;
                        __hip_atomic_store(pa.sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        sm.ctl[0] = 1;
                    } else {
                        // mpe_fused_observe's step of cycle c from the state of cycle c - 1 (same operations, same order)
                        const int t0 = 3 * (c - 1);
                        const bool stepped = t0 + 2 < limit;
                        double r_good = 0.0, r_adv = 0.0;
                        if (stepped) {
                            const int a0 = w0 & 0xff, a1 = w1 & 0xff, a2 = w2 & 0xff;
                            if (slot == COEVO_SLOT_ADVERSARY) mpe_world_step(s, a0, a1, a2, a.pos_first, r_good, r_adv);
                            else mpe_world_move(s, a0, a1, a2, a.pos_first);
                        }
                        if (slot == COEVO_SLOT_ADVERSARY) {   // the game's owner row keeps the books
                            double rg_prev = sm.gs[l][18], a_adv = sm.gs[l][19], a_a0 = sm.gs[l][20], a_a1 = sm.gs[l][21];
                            if (t0 < limit) a_adv = a_adv + rg_prev;
                            if (t0 + 1 < limit) a_a0 = a_a0 + rg_prev;
                            if (stepped) { a_a1 = a_a1 + r_adv; rg_prev = r_good; }
                            sm.gs[l][18] = rg_prev; sm.gs[l][19] = a_adv; sm.gs[l][20] = a_a0; sm.gs[l][21] = a_a1;
                        }
                        game_moved_to_lds(sm.gs[l], s);
                    }
                }
                mpe_obs_from_game(s, slot, o);
#pragma unroll
                for (int k = 0; k < 10; ++k)
                    if (!__builtin_isfinite(o[k])) st |= COEVO_ST_BAD_INPUT;
            }
#pragma unroll
            for (int k = 0; k < COEVO_OBS_STRIDE; ++k) sm.xs0[l][k] = o[k];
        }
        prefetch();
        }
        if (a.stamps && t == 0)
            atomicMin(&a.stamps[2 * (COEVO_STAMP_SLOTS * (size_t)c + blockIdx.x % COEVO_STAMP_SLOTS)],
                      (unsigned long long)__builtin_amdgcn_s_memrealtime());
        __syncthreads();   // (cycle 0: waits for the LDS-DMA too)
        if (sm.ctl[0]) break;   // workgroup-uniform

        // ---- fc1 (v_mfma_f32_4x4x1, rows in groups of four) ---------------------------------------------------------------
        const float *b1s = sm.par + D * H1;
        f32x4_acc c0[NG], c1[NG];
        {
            const float bia = b1s[t], bib = b1s[t + 256];
#pragma unroll
            for (int gq = 0; gq < NG; ++gq)
#pragma unroll
                for (int i = 0; i < 4; ++i) { c0[gq][i] = bia; c1[gq][i] = bib; }
            float4 xk[NG][3];
#pragma unroll
            for (int gq = 0; gq < NG; ++gq)
#pragma unroll
                for (int j = 0; j < 3; ++j) xk[gq][j] = *reinterpret_cast<const float4 *>(&sm.xs0[4 * gq + (l & 3)][4 * j]);
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                if (k < D) {   // wave-uniform
                    const float wa = sm.par[k * H1 + t], wb = sm.par[k * H1 + 256 + t];
#pragma unroll
                    for (int gq = 0; gq < NG; ++gq) {
                        const float4 xv = xk[gq][k >> 2];
                        const float x = (k & 3) == 0 ? xv.x : (k & 3) == 1 ? xv.y : (k & 3) == 2 ? xv.z : xv.w;
                        c0[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(x, wa, c0[gq], 0, 0, 0);
                        c1[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(x, wb, c1[gq], 0, 0, 0);
                    }
                }
            }
        }
        const float p_g1a = b1s[H1 + t], p_g1b = b1s[H1 + t + 256], p_be1a = b1s[2 * H1 + t], p_be1b = b1s[2 * H1 + t + 256];
        // ---- LayerNorm(512) + ReLU ------------------------------------------------------------------------------------------
        float v[2 * R];
#pragma unroll
        for (int r = 0; r < R; ++r) { v[2 * r] = c0[r >> 2][r & 3]; v[2 * r + 1] = c1[r >> 2][r & 3]; }
        ln_block_sums<2 * R>(v, sm.red, w, l);
        __syncthreads();
        const int lr = l < R ? l : R - 1;
        ln_center<R, 2>(v, sm.red, sm.red2, w, l, lr);
        __syncthreads();
        st = ln512_relu_store<R, true>(sm, v, lr, nrows, p_g1a, p_g1b, p_be1a, p_be1b, st);
        asm volatile("" : "+v"(st));
        __syncthreads();

        // ---- fc2 on the vector ALU (FC2_DPP) ----------------------------------------------------------------------------------
        float u[R];
        {
            const float p_b2 = sm.p2[0][t];
#pragma unroll
            for (int r = 0; r < R; ++r) u[r] = p_b2;
        }
        {
            const float *xrow = &sm.h1r[0][l & 15];
            auto issue_s = [&](float4 (&buf)[US], int kq) {
#pragma unroll
                for (int uu = 0; uu < US; ++uu) buf[uu] = wps[(size_t)(kq + uu) * 64];
            };
            auto consume_s = [&](const float4 (&buf)[US], int kq) {
#pragma unroll
                for (int b = 0; b < US / 4; ++b) {
                    float xv[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) xv[r] = xrow[r * H1 + 4 * (kq + 4 * b)];
                    fmac_block16<R>(u, xv, buf[4 * b], buf[4 * b + 1], buf[4 * b + 2], buf[4 * b + 3]);
                }
            };
#pragma nounroll
            for (int kq = 0; kq < 128; kq += 2 * US) {
                consume_s(sbufA, kq);
                if (kq + 2 * US < 128) issue_s(sbufA, kq + 2 * US);   // wave-uniform
                __builtin_amdgcn_sched_barrier(0);
                consume_s(sbufB, kq + US);
                if (kq + 3 * US < 128) issue_s(sbufB, kq + 3 * US);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- LayerNorm(256) + ReLU ------------------------------------------------------------------------------------------
        ln_block_sums<R>(u, sm.red, w, l);
        __syncthreads();
        {
            const float tot = ((sm.red[0][lr] + sm.red[1][lr]) + sm.red[2][lr]) + sm.red[3][lr];
            const float meanv = tot * (1.0f / H2);
#pragma unroll
            for (int r = 0; r < R; ++r) u[r] = u[r] - __int_as_float(__builtin_amdgcn_readlane(__float_as_int(meanv), r));
            float sq[R];
#pragma unroll
            for (int r = 0; r < R; ++r) sq[r] = u[r] * u[r];
            const float s = packed_totals<R>(sq, l);
            if (l < R) sm.red2[w][l] = s;
        }
        __syncthreads();
        {
            const float rstdv = ln256_rstd(sm.red2, lr);
            const float p_g2 = sm.p2[1][t], p_be2 = sm.p2[2][t];
            st = ln256_relu_store<R>(u, rstdv, nrows, p_g2, p_be2, sm.h2, st);
        }
        asm volatile("" : "+v"(st));
        __syncthreads();

        // ---- output layer + first-max action: wave 0; the action is posted as the tagged word -------------------------------
        if (w == 0) {
            if (l < R * NACT) {
                const int r = l / NACT, o = l % NACT;
                const float y = out_chain<8>(sm.pb3[o], &sm.w3s[o][0], &sm.h2[r][0]);
                sm.logit[r][o] = y;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (l < nrows) {   // strict '>' scan from -inf
                const FirstMax fm = first_max_action(sm.logit[l], st);
                const int best = fm.best;
                st = fm.st;
                const int g = sm.rowinfo[l][0], slot = sm.rowinfo[l][1];
                __hip_atomic_store(tags + (size_t)(c & 1) * 3 * N + 3 * (size_t)(g + zero) + slot, ((c + 1) << 8) | best, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                if (c == pa.n_cycles - 1) pa.act_plain[(size_t)(c & 1) * 3 * N + 3 * (size_t)(g + zero) + slot] = best;
                if (a.logits) {
                    int r0 = row0;
                    asm volatile("" : "+s"(r0));   // (not an address to carry through the loop)
#pragma unroll
                    for (int o = 0; o < NACT; ++o) a.logits[(size_t)(r0 + l) * COEVO_LOGIT_STRIDE + o] = sm.logit[l][o];
                }
            }
        }
        if (a.stamps && t == 0)
            atomicMax(&a.stamps[2 * (COEVO_STAMP_SLOTS * (size_t)c + blockIdx.x % COEVO_STAMP_SLOTS) + 1],
                      (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
    // what the last per-cycle launch leaves for coevo_mpe_final_step: the state of cycle n_cycles - 1 + the books, in that
    // cycle's buffer, written by each game's owner row (cycle 0 writes nothing: its state is the reset state in buffer 0)
    if (w == 0 && l < nrows && sm.rowinfo[l][1] == COEVO_SLOT_ADVERSARY && pa.n_cycles > 1 && !sm.ctl[0]) {
        const int g = sm.rowinfo[l][0];
        double *sn = ((pa.n_cycles - 1) & 1) ? pa.state_alt : const_cast<double *>(a.state);
#pragma unroll
        for (int f = 0; f < 22; ++f) sn[(size_t)f * N + g] = sm.gs[l][f];
    }
    // ... and, asked to, the closing step itself (mpe_final_step_kernel, operation for operation): the owner row waits for the
    // last cycle's three actions, credits the last rewards and writes the game's return triple (+ the all-gather record)
    if (pa.rewards && w == 0 && l < nrows && sm.rowinfo[l][1] == COEVO_SLOT_ADVERSARY && !sm.ctl[0]) {
        const int g = sm.rowinfo[l][0], limit = sm.rowinfo[l][2], cyc = pa.n_cycles - 1;
        const int32_t *tp = tags + (size_t)(cyc & 1) * 3 * N + 3 * (size_t)g;
        const TaggedWords tw = wait_tagged_actions(tp, pa.sync, cyc + 1);
        const int w0 = tw.w0, w1 = tw.w1, w2 = tw.w2;
        if (!tw.ok) {
            st |= COEVO_ST_SYNC_TIMEOUT;
            __hip_atomic_store(pa.sync, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            double a_adv = sm.gs[l][19], a_a0 = sm.gs[l][20], a_a1 = sm.gs[l][21];
            const int t0 = 3 * cyc;
            const double rg_prev = sm.gs[l][18];
            if (t0 < limit) a_adv = a_adv + rg_prev;
            if (t0 + 1 < limit) a_a0 = a_a0 + rg_prev;
            if (t0 + 2 < limit) {
                MpeGame s;
                game_from_lds(sm.gs[l], s);
                double r_good, r_adv;
                mpe_world_step(s, w0 & 0xff, w1 & 0xff, w2 & 0xff, a.pos_first, r_good, r_adv);
                a_a1 = a_a1 + r_adv;
            }
            pa.rewards[3 * (size_t)g + 0] = a_a0;
            pa.rewards[3 * (size_t)g + 1] = a_a1;
            pa.rewards[3 * (size_t)g + 2] = a_adv;
            const coevo_final_pack &pk = pa.pack;
            if (pk.out && g < pk.n_roles * pk.n_local * pk.hof && g % pk.hof == pk.hof - 1) {
                const int ij = g / pk.hof, role = ij / pk.n_local, j = ij % pk.n_local;
                double *o = pk.out + 4 * (size_t)ij;
                o[0] = a_a0;
                o[1] = a_a1;
                o[2] = a_adv;
                o[3] = (double)pk.dist[(size_t)role * pk.dist_pitch + pk.dist_first + j];
            }
        }
    }
    if (st) atomicOr(a.status, st);
}

}  // namespace coevo
