// K1 - FCNetwork policy step for many (weight set x observation rows) tasks in one launch.
//
// Replaces FCNetwork.forward + determine_action (reference MPE/fcnetwork.py:37-90), which the reference calls
// once per agent-step at batch 1 (utils/game_logic_functions.py:152-163).
//
// One workgroup (4 wavefronts of 64) = one task = one weight set applied to up to R observation rows.
// HBM traffic per task is the weight set itself, read exactly once, fully coalesced:
//   fc1  W1t[k][512]           each lane owns outputs t and t+256, wave reads 256 B rows (20 KB total)
//   fc2  W2q[4][128][64][4]    wave w streams its 128 KiB block as 1 KiB wave-instructions (global_load_dwordx4),
//                              8-16 in flight per lane; each 16-byte piece is 4 k of the lane's own output column and
//                              feeds v_mfma_f32_4x4x1_16B_f32 directly (16 blocks x 4 columns = the wave's 64 columns,
//                              4 rows, one k per instruction); the A operands of a row group are one ds_read_b128
//   out  W3[5][256]            staged through LDS once
// Arithmetic per weight byte is tiny (R FMAs per 4 bytes), but as VALU FMAs fed by LDS broadcasts it still cost a lone
// workgroup 27 us per net against ~5 us of HBM time (round 1 probe; the stream rate of one CU: tools/stream_waves_probe.hip): the matrix pipe, otherwise idle here,
// does the same sequential-k fma chains (tools/mfma4_chain_probe.hip: bit-identical) in far fewer issue slots and LDS
// reads.  (v_mfma_f32_16x16x4_f32, tools/mfma16_chain_probe.hip, is exact as well but spends 16 tile rows on <= 8.)
// All fp32 math follows the canonical order in coevo_common.hip.h, so logits equal the oracle's bit for bit.
//
// Five forward bodies, one header each, all in THIS translation unit (what else is in the module reaches the scheduler:
// profiles/r29_fc_forward_headers.md):
//   fc_body_unrolled.hip.h        fc_policy_body          per-individual nets, P per workgroup (32-row cycle kernel, MODE_OBS / MODE_STATE)
//   fc_body_compact.hip.h         fc_policy_body_c        per-individual nets, few issued instructions; fc2 on MFMA or the vector ALU
//   fc_body_mfma32.hip.h          fc_policy_mfma_body     shared opponents, up to 32 rows on v_mfma_f32_32x32x2
//   fc_body_mfma16.hip.h          fc_policy_mfma16_body   shared opponents, up to 16 rows on v_mfma_f32_16x16x4
//   fc_rollout_persistent.hip.h   fc_rollout_small_kernel a whole rollout of a small launch in one persistent launch
// What they run the same way AND the compiler turns into the same code either way is written once, in fc_forward_common.hip.h
// (out_chain, first_max_action, store_action, fc2_mfma4_consume, the packed LayerNorm passes of the two lean forms) and in
// fc_rollout_persistent.hip.h (the persistent kernel's game copy and tagged-word wait); the other phases are still spelled out
// per body - profiles/r12_fc_forward_helpers.md has the measurements behind that line.  Here: the kernels that pick a body, the
// launch-form policy and the C entry points.
#include <cstdlib>
#include <type_traits>

#include "fc_forward_common.hip.h"
#include "fc_body_unrolled.hip.h"
#include "fc_body_compact.hip.h"
#include "fc_body_mfma32.hip.h"
#include "fc_body_mfma16.hip.h"
#include "fc_rollout_persistent.hip.h"

namespace coevo {

template <int R, int MODE>
__global__ __launch_bounds__(256) void fc_policy_kernel(FcArgs a)
{
    stamp_begin(a.stamps);
    if constexpr (MODE == MODE_FUSED) {   // fused env step: the body built for few instructions
        __shared__ __attribute__((aligned(16))) FcSmemC<R> smc;
        fc_policy_body_c<R, MODE>(a, smc, a.tasks, blockIdx.x, gridDim.x);
    } else {
        __shared__ __attribute__((aligned(16))) FcSmem<R, 1> sm;
        fc_policy_body<R, MODE, 1>(a, sm, a.tasks, blockIdx.x, gridDim.x);
    }
    stamp_end(a.stamps);
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void fc_policy_mfma_kernel(FcArgs a)
{
    __shared__ __attribute__((aligned(16))) FcMfmaSmem sm;
    fc_policy_mfma_body<MODE>(a, sm, a.tasks[blockIdx.x]);
}

// The lean merged cycle launch: shared-opponent tasks of <= 16 rows (fc_policy_mfma16_body) + one per-individual net per
// streaming workgroup, four workgroups per CU.
template <int R, int MODE = MODE_FUSED>
__global__ __launch_bounds__(256, 4) void fc_cycle16_kernel(FcArgs a)
{
    // (16-byte alignment stated: hipcc otherwise assumes 4 and splits every ds_read_b128 of the k-quad image into two
    // ds_read2_b32 with a vector add each - a third of a vector instruction per MFMA in the stream loop)
    __shared__ __attribute__((aligned(16))) union Cycle16Smem {
        FcMfma16Smem heavy;
        FcSmemC<R> light;
    } sm;
    static_assert(sizeof(sm) <= 40960, "four workgroups per CU");
    stamp_begin(a.stamps);
    if ((int)blockIdx.x < a.n_heavy)  // workgroup-uniform
        fc_policy_mfma16_body<MODE>(a, sm.heavy, a.tasks[blockIdx.x]);
    else {
        const int li = (int)blockIdx.x - a.n_heavy;
        // the device-env launch only: a resident net is read with plain loads (workgroup-uniform, once per workgroup)
        if (MODE == MODE_FUSED && li < a.n_light && (a.light_tasks[li].reserved & COEVO_TASK_RESIDENT))
            fc_policy_body_c<R, MODE, FC2_MFMA, MODE == MODE_FUSED>(a, sm.light, a.light_tasks, li, a.n_light);
        else
            fc_policy_body_c<R, MODE>(a, sm.light, a.light_tasks, li, a.n_light);
    }
    stamp_end(a.stamps);
}

// The SMALL merged cycle launch: every task (shared-opponent chunk or per-individual net) has <= 8 rows and runs the
// per-individual body with its fc2 on the vector ALU (FC2_DPP).  For launches that leave CUs idle - one rank of a population
// sharded over 4 / 8 GPUs (genetic_algorithm.py:125-217 split by index: 25 or 50 individuals per role), a cohort of the
// host-stepped env - where a workgroup's life, not bytes, is the launch's duration.  <= 256 registers: two workgroups per CU.
template <int R, int MODE = MODE_FUSED>
__global__ __launch_bounds__(256, 2) void fc_cycle_small_kernel(FcArgs a)
{
    __shared__ __attribute__((aligned(16))) FcSmemC<R> sm;
    stamp_begin(a.stamps);
    const bool heavy = (int)blockIdx.x < a.n_heavy;   // workgroup-uniform
    fc_policy_body_c<R, MODE, FC2_DPP>(a, sm, heavy ? a.tasks : a.light_tasks, heavy ? (int)blockIdx.x : (int)blockIdx.x - a.n_heavy,
                                       heavy ? a.n_heavy : a.n_light);
    stamp_end(a.stamps);
}

// One launch = one env-cycle of one cohort of games (fused env step): the shared-opponent tasks first (lowest block
// indices: they are dispatched first and are the longer workgroups), then the per-individual tasks.  Both kinds of
// workgroup get the MFMA path's footprint (<= 256 registers, ~73 KiB LDS: two workgroups per CU), so a launch of a
// few hundred workgroups occupies the CUs in waves - together with a second cohort's launch on another stream the
// CUs' weight streams run out of phase and HBM stays busy through the non-streaming phases of any one workgroup.
template <int R, int P>
__global__ __launch_bounds__(256, 2) void fc_cycle_kernel(FcArgs a)
{
    __shared__ __attribute__((aligned(16))) union CycleSmem {
        FcMfmaSmem heavy;
        FcSmem<R, P> light;
    } sm;
    stamp_begin(a.stamps);
    if ((int)blockIdx.x < a.n_heavy)  // workgroup-uniform
        fc_policy_mfma_body<MODE_FUSED>(a, sm.heavy, a.tasks[blockIdx.x]);
    else
        fc_policy_body<R, MODE_FUSED, P>(a, sm.light, a.light_tasks, P * ((int)blockIdx.x - a.n_heavy), a.n_light);
    stamp_end(a.stamps);
}

// The row-count instantiations of the per-individual kernels: f(R) is called with R = 1, 2, 5 or 8 as a compile-time
// constant (std::integral_constant), the smallest that holds `rows`
template <class F>
static void dispatch_rows(int rows, F &&f)
{
    if (rows <= 1) f(std::integral_constant<int, 1>{});
    else if (rows <= 2) f(std::integral_constant<int, 2>{});
    else if (rows <= 5) f(std::integral_constant<int, 5>{});
    else f(std::integral_constant<int, 8>{});
}

// compute units of the device that is current at the first call, asked once (every device of a process is assumed to be
// the same part); 0: the query failed
static int device_cu_count()
{
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            return 0;
        cus = n;
    }
    return cus;
}

template <int MODE>
static int launch_fc(const FcArgs &a, int n_tasks, int max_rows, hipStream_t s)
{
    if (n_tasks <= 0) return COEVO_OK;
    if (max_rows <= 8)
        dispatch_rows(max_rows, [&](auto R) {
            hipLaunchKernelGGL((fc_policy_kernel<decltype(R)::value, MODE>), dim3(n_tasks), dim3(256), 0, s, a);
        });
    else
        hipLaunchKernelGGL((fc_policy_mfma_kernel<MODE>), dim3(n_tasks), dim3(256), 0, s, a);
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

}  // namespace coevo

#ifdef COEVO_PHASE_STAMPS
extern "C" int coevo_debug_read_wave_stamps(unsigned long long *host_out, int n_words)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(coevo::g_wave_stamps), sizeof(unsigned long long) * n_words) ==
                   hipSuccess ? 0 : -2;
}

extern "C" int coevo_debug_read_phase_stamps(unsigned long long *host_out, int n_words)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(coevo::g_phase_stamps), sizeof(unsigned long long) * n_words) ==
                   hipSuccess ? 0 : -2;
}
#endif

static bool rows_outside(int max_rows, int limit) { return max_rows < 1 || max_rows > limit; }

// what every fused env-step launch refuses: a missing buffer, or a cycle that would read the buffer it writes
static bool bad_fused_cycle(const double *state_prev, double *state_next, int n_games, const int32_t *row_game,
                            const int32_t *row_slot, const int32_t *act_prev, int32_t *act_cur, int cycle, int32_t *status)
{
    return !state_prev || !state_next || !row_game || !row_slot || !act_prev || !act_cur || !status || n_games <= 0 ||
           cycle < 0 || state_prev == state_next || act_prev == act_cur;
}

// The launch arguments of an env-cycle with the env step fused in (the persistent rollout: the reset state, no cycle and no
// action buffers).  Here and in every entry: fields by name, every field a launch mode does not name stays zero.
static coevo::FcArgs fused_args(const float *slab, const coevo_fc_task *tasks, const double *state_prev, double *state_next,
                                int n_games, const int32_t *row_game, const int32_t *row_slot, const int32_t *act_prev,
                                int32_t *act_cur, const int32_t *game_limit, int cycle, int pos_first, int32_t *status,
                                uint64_t *stamps)
{
    coevo::FcArgs a{};
    a.slab = slab; a.tasks = tasks; a.state = state_prev; a.row_game = row_game; a.row_slot = row_slot; a.n_games = n_games;
    a.status = status; a.stamps = reinterpret_cast<unsigned long long *>(stamps); a.state_next = state_next;
    a.act_prev = act_prev; a.act_cur = act_cur; a.game_limit = game_limit; a.cycle = cycle; a.pos_first = pos_first;
    return a;
}

extern "C" int coevo_fc_forward_argmax(const float *slab, const coevo_fc_task *tasks, int n_tasks,
                                       int max_rows_per_task, const float *obs, int32_t *actions, float *logits,
                                       int32_t *status, void *stream)
{
    if (!slab || !tasks || !obs || !actions || !status || n_tasks < 0) return COEVO_ERR_ARG;
    if (rows_outside(max_rows_per_task, COEVO_FC_MAX_ROWS)) return COEVO_ERR_ARG;
    coevo::FcArgs a{};
    a.slab = slab; a.tasks = tasks; a.obs = obs; a.actions = actions; a.logits = logits; a.status = status;
    return coevo::launch_fc<coevo::MODE_OBS>(a, n_tasks, max_rows_per_task, (hipStream_t)stream);
}

extern "C" int coevo_mpe_policy_cycle_stamped(const float *slab, const coevo_fc_task *tasks, int n_tasks,
                                              int max_rows_per_task, const double *state, int n_games,
                                              const int32_t *row_game, const int32_t *row_slot, int32_t *actions,
                                              int32_t *status, uint64_t *stamps, void *stream)
{
    if (!slab || !tasks || !state || !row_game || !row_slot || !actions || !status) return COEVO_ERR_ARG;
    if (n_tasks < 0 || n_games <= 0) return COEVO_ERR_ARG;
    if (rows_outside(max_rows_per_task, COEVO_FC_MAX_ROWS)) return COEVO_ERR_ARG;
    coevo::FcArgs a{};
    a.slab = slab; a.tasks = tasks; a.state = state; a.row_game = row_game; a.row_slot = row_slot; a.n_games = n_games;
    a.actions = actions; a.status = status; a.stamps = reinterpret_cast<unsigned long long *>(stamps);
    return coevo::launch_fc<coevo::MODE_STATE>(a, n_tasks, max_rows_per_task, (hipStream_t)stream);
}

extern "C" int coevo_mpe_policy_cycle(const float *slab, const coevo_fc_task *tasks, int n_tasks,
                                      int max_rows_per_task, const double *state, int n_games,
                                      const int32_t *row_game, const int32_t *row_slot, int32_t *actions,
                                      int32_t *status, void *stream)
{
    return coevo_mpe_policy_cycle_stamped(slab, tasks, n_tasks, max_rows_per_task, state, n_games, row_game, row_slot,
                                          actions, status, nullptr, stream);
}

extern "C" int coevo_mpe_policy_cycle_fused(const float *slab, const coevo_fc_task *tasks, int n_tasks,
                                            int max_rows_per_task, const double *state_prev, double *state_next,
                                            int n_games, const int32_t *row_game, const int32_t *row_slot,
                                            const int32_t *act_prev, int32_t *act_cur, const int32_t *game_limit,
                                            int cycle, int pos_first, int32_t *status, uint64_t *stamps, void *stream)
{
    if (!slab || !tasks || n_tasks < 0 || rows_outside(max_rows_per_task, COEVO_FC_MAX_ROWS) ||
        bad_fused_cycle(state_prev, state_next, n_games, row_game, row_slot, act_prev, act_cur, cycle, status))
        return COEVO_ERR_ARG;
    const coevo::FcArgs a = fused_args(slab, tasks, state_prev, state_next, n_games, row_game, row_slot, act_prev, act_cur,
                                       game_limit, cycle, pos_first, status, stamps);
    return coevo::launch_fc<coevo::MODE_FUSED>(a, n_tasks, max_rows_per_task, (hipStream_t)stream);
}

// Which kernel a merged cycle launch of this shape runs (the launcher's own decision, exposed for tests and bench records)
extern "C" int coevo_mpe_cycle_kernel_form(int n_heavy, int n_light, int heavy_max_rows, int light_max_rows,
                                           int concurrent_launches)
{
    if (n_heavy <= 0 || n_light <= 0 || light_max_rows < 1 || light_max_rows > 8) return COEVO_ERR_ARG;
    // workgroup slots of the 32-row kernel: two per CU (<= 256 registers, ~73 KiB LDS)
    const int slots = 2 * coevo::device_cu_count();
    if (slots <= 0) return COEVO_ERR_HIP;
    const int conc = concurrent_launches > 1 ? concurrent_launches : 1;
    const int wgs = (n_heavy + n_light) * conc;
    // every task of <= 8 rows and no more workgroups in flight than CUs: the small-launch kernel (COEVO_SMALL_KERNEL=0: A/B).
    // (Two per CU share their SIMDs' vector ALU: a rank of 4 - 360 workgroups of <= 8 rows - 27.6-30.5 us per launch against
    // 21.8 for the lean kernel's 270 with 16-row matrix-core tiles; a rank of 8 - 231 - 16.4 against 21.0.)
    static const char *const small_env = getenv("COEVO_SMALL_KERNEL");
    static const bool small_ok = !(small_env && small_env[0] == '0');
    if (small_ok && heavy_max_rows >= 1 && heavy_max_rows <= 8 && 2 * wgs <= slots) return COEVO_CYCLE_FORM_SMALL;
    if (heavy_max_rows >= 1 && heavy_max_rows <= 16 && wgs <= 2 * slots) return COEVO_CYCLE_FORM_LEAN16;
    // If one net per streaming workgroup does not fit the slots in a single round, pair the nets: the second round would
    // otherwise wait for the slots of the (long) shared-opponent workgroups.
    return wgs > slots ? COEVO_CYCLE_FORM_TILE32_PAIRED : COEVO_CYCLE_FORM_TILE32;
}

// The persistent launch needs every workgroup resident at once: <= 256 registers and < 80 KiB of LDS, so two fit a CU.  (With
// more than one per CU the rollout is bound by what ONE CU streams - ~47 GB/s, tools/stream_waves_probe.hip: two 0.56 MB nets
// per cycle = 20 us - and still ahead of the per-cycle launches of the lean kernel: a rank of 4, 450 workgroups, 20.2 against
// 23.3 us per cycle.)
extern "C" int coevo_mpe_persistent_fits(int n_heavy, int n_light, int heavy_max_rows, int light_max_rows, int concurrent_launches)
{
    // (either list may be empty: the ten evaluation games of Co-ES are six per-individual tasks and nothing else)
    if (n_heavy < 0 || n_light < 0 || n_heavy + n_light <= 0) return COEVO_ERR_ARG;
    if ((n_light > 0 && (light_max_rows < 1 || light_max_rows > 8)) || (n_heavy > 0 && heavy_max_rows < 1)) return COEVO_ERR_ARG;
    if (n_heavy > 0 && heavy_max_rows > 8) return 0;
    const int cus = coevo::device_cu_count();
    if (cus <= 0) return COEVO_ERR_HIP;
    // what the runtime says the instantiation's residency is (two per CU as built; asked, not assumed: a launch that is not
    // all resident would wait for itself)
    const int hr = n_heavy > 0 ? heavy_max_rows : 0, lr = n_light > 0 ? light_max_rows : 0, rows = hr > lr ? hr : lr;
    static int per_cu_of[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};   // by the instantiation's R
    int per_cu = -1;
    coevo::dispatch_rows(rows, [&](auto R) {
        constexpr int RR = decltype(R)::value;
        if (per_cu_of[RR] < 0) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, coevo::fc_rollout_small_kernel<RR>, 256, 0) == hipSuccess)
                per_cu_of[RR] = n > 2 ? 2 : n;   // (never more than the two the kernel was sized for)
        }
        per_cu = per_cu_of[RR];
    });
    if (per_cu < 0) return COEVO_ERR_HIP;
    const int conc = concurrent_launches > 1 ? concurrent_launches : 1;
    return (n_heavy + n_light) * conc <= per_cu * cus ? 1 : 0;
}

extern "C" int coevo_mpe_persistent_sync_words(int n_games) { return n_games > 0 ? 4 + 6 * n_games : COEVO_ERR_ARG; }

extern "C" int coevo_mpe_rollout_persistent(const float *slab, const coevo_fc_task *heavy_tasks, int n_heavy,
                                            const coevo_fc_task *light_tasks, int n_light, int light_max_rows, int heavy_max_rows,
                                            double *state, double *state_alt, int n_games, const int32_t *row_game,
                                            const int32_t *row_slot, int32_t *actions_by_game, const int32_t *game_limit,
                                            int n_cycles, int pos_first, int32_t *status, uint64_t *stamps, int32_t *sync_words,
                                            int concurrent_launches, double *rewards, const coevo_final_pack *pack,
                                            int sync_cleared, void *stream)
{
    if (!slab || (n_heavy > 0 && !heavy_tasks) || (n_light > 0 && !light_tasks) || !state || !state_alt || state == state_alt ||
        !row_game || !row_slot || !actions_by_game || !status || !sync_words || n_games <= 0 || n_cycles < 1 || n_cycles > (1 << 22))
        return COEVO_ERR_ARG;
    const int fits = coevo_mpe_persistent_fits(n_heavy, n_light, heavy_max_rows, light_max_rows, concurrent_launches);
    if (fits < 0) return fits;
    if (!fits) return COEVO_ERR_UNSUPPORTED;   // not all resident at once: the per-cycle launches
    hipStream_t s = (hipStream_t)stream;
    // (a kernel, not hipMemsetAsync: captured into a hipGraph and replayed after other work had run, the memset node of this
    // runtime left device pointers in the buffer - the Co-ES evaluation rollout timed out on them)
    if (!sync_cleared) {
        hipLaunchKernelGGL(coevo::sync_clear_kernel, dim3((4 + 6 * n_games + 255) / 256), dim3(256), 0, s, sync_words, 4 + 6 * n_games);
        COEVO_HIP_CHECK(hipGetLastError());
    }
    coevo::FcArgs a = fused_args(slab, heavy_tasks, state, nullptr, n_games, row_game, row_slot, nullptr, nullptr, game_limit, 0,
                                 pos_first, status, stamps);
    a.light_tasks = light_tasks; a.n_heavy = n_heavy; a.n_light = n_light;
    if (pack && (!rewards || !pack->out || !pack->dist || pack->n_roles < 1 || pack->n_local < 1 || pack->hof < 1 ||
                 (int64_t)pack->n_roles * pack->n_local * pack->hof > n_games || pack->dist_first < 0 ||
                 pack->dist_first + pack->n_local > pack->dist_pitch))
        return COEVO_ERR_ARG;
    const coevo::PersistArgs pa{n_cycles, sync_words, state_alt, actions_by_game, rewards, pack ? *pack : coevo_final_pack{}};
    const int hr = n_heavy > 0 ? heavy_max_rows : 0, lr = n_light > 0 ? light_max_rows : 0;
    const int rows = hr > lr ? hr : lr;
    const dim3 grid(n_heavy + n_light), block(256);
    coevo::dispatch_rows(rows, [&](auto R) {
        hipLaunchKernelGGL((coevo::fc_rollout_small_kernel<decltype(R)::value>), grid, block, 0, s, a, pa);
    });
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

extern "C" int coevo_mpe_policy_cycle_merged(const float *slab, const coevo_fc_task *heavy_tasks, int n_heavy,
                                             const coevo_fc_task *light_tasks, int n_light, int light_max_rows,
                                             const double *state_prev, double *state_next, int n_games,
                                             const int32_t *row_game, const int32_t *row_slot, const int32_t *act_prev,
                                             int32_t *act_cur, const int32_t *game_limit, int cycle, int pos_first,
                                             int32_t *status, uint64_t *stamps, int concurrent_launches,
                                             int heavy_max_rows, void *stream)
{
    if (!slab || !heavy_tasks || !light_tasks || n_heavy <= 0 || n_light <= 0 || rows_outside(light_max_rows, 8) ||
        bad_fused_cycle(state_prev, state_next, n_games, row_game, row_slot, act_prev, act_cur, cycle, status))
        return COEVO_ERR_ARG;
    coevo::FcArgs a = fused_args(slab, heavy_tasks, state_prev, state_next, n_games, row_game, row_slot, act_prev, act_cur,
                                 game_limit, cycle, pos_first, status, stamps);
    a.light_tasks = light_tasks; a.n_heavy = n_heavy; a.n_light = n_light;
    const int form = coevo_mpe_cycle_kernel_form(n_heavy, n_light, heavy_max_rows, light_max_rows, concurrent_launches);
    if (form < 0) return form;
    hipStream_t s = (hipStream_t)stream;
    const bool pair = form == COEVO_CYCLE_FORM_TILE32_PAIRED;
    // (only the paired 32-row form carries two nets per streaming workgroup: n_heavy + n_light workgroups in every other form)
    const dim3 grid(n_heavy + (pair ? (n_light + 1) / 2 : n_light)), block(256);
    if (form == COEVO_CYCLE_FORM_SMALL) {
        coevo::dispatch_rows(heavy_max_rows > light_max_rows ? heavy_max_rows : light_max_rows, [&](auto R) {
            hipLaunchKernelGGL((coevo::fc_cycle_small_kernel<decltype(R)::value>), grid, block, 0, s, a);
        });
    } else if (form == COEVO_CYCLE_FORM_LEAN16) {
        // the lean kernel: four workgroups per CU hold everything at one net per streaming workgroup
        coevo::dispatch_rows(light_max_rows, [&](auto R) {
            hipLaunchKernelGGL((coevo::fc_cycle16_kernel<decltype(R)::value>), grid, block, 0, s, a);
        });
    } else {
        // (when not everything fits - Co-ES with 3000 nets - the 32-row tiles with two nets per streaming workgroup are
        // ahead: 109 vs 106 generations/s)
        coevo::dispatch_rows(light_max_rows, [&](auto R) {
            if (pair) hipLaunchKernelGGL((coevo::fc_cycle_kernel<decltype(R)::value, 2>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((coevo::fc_cycle_kernel<decltype(R)::value, 1>), grid, block, 0, s, a);
        });
    }
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

// The merged launch with the observations GIVEN (the env stepped elsewhere - on the host cores, env_mode "host"): shared-opponent
// tasks (<= 16 rows) and per-individual tasks (<= 8 rows) of one env-cycle in one launch of the lean kernel, instead of one
// coevo_fc_forward_argmax per task class.  Needs every workgroup resident at four per CU; COEVO_ERR_ARG otherwise (the caller
// then launches the classes one after the other).
extern "C" int coevo_fc_forward_merged(const float *slab, const coevo_fc_task *heavy_tasks, int n_heavy, int heavy_max_rows,
                                       const coevo_fc_task *light_tasks, int n_light, int light_max_rows, const float *obs,
                                       int32_t *actions, float *logits, int32_t *status, void *stream)
{
    if (!slab || !heavy_tasks || !light_tasks || !obs || !actions || !status) return COEVO_ERR_ARG;
    if (n_heavy <= 0 || n_light <= 0 || rows_outside(heavy_max_rows, 16) || rows_outside(light_max_rows, 8)) return COEVO_ERR_ARG;
    const int cus = coevo::device_cu_count();
    if (cus <= 0) return COEVO_ERR_HIP;
    if (n_heavy + n_light > 4 * cus) return COEVO_ERR_ARG;
    coevo::FcArgs a{};
    a.slab = slab; a.tasks = heavy_tasks; a.obs = obs; a.actions = actions; a.logits = logits; a.status = status;
    a.light_tasks = light_tasks; a.n_heavy = n_heavy; a.n_light = n_light;
    const dim3 grid(n_heavy + n_light), block(256);
    hipStream_t s = (hipStream_t)stream;
    coevo::dispatch_rows(light_max_rows, [&](auto R) {
        hipLaunchKernelGGL((coevo::fc_cycle16_kernel<decltype(R)::value, coevo::MODE_OBS>), grid, block, 0, s, a);
    });
    COEVO_HIP_CHECK(hipGetLastError());
    return COEVO_OK;
}

COEVO_DEFINE_TU_FLAGS(fc_forward)
