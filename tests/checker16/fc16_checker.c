/*
 * fc16_checker.c - TEST INFRASTRUCTURE ONLY: the float16 FCNetwork forward restated in plain sequential C, and
 * play_game's AEC bookkeeping around it (the same bookkeeping as oracle_play_game in oracle/coevo_oracle.c).
 *
 * The float16 contract (DESIGN.md "float16 nets"; coevonet_amd/csrc/fc16.hip reproduces it bit for bit):
 *   x = f16(obs); Linear: acc = b; acc = fmaf(w, x, acc) in k order, y = f16(acc)  (w, x fp16: every product is exact, so
 *   the Linear layers need no FMA - fmaf is kept for symmetry with the canonical rule); LayerNorm: the canonical fp32 rule
 *   (blocks of 64, adjacent-pairs tree, block sums left to right) on the fp16 inputs, output f16; ReLU; logits f16;
 *   first maximum by a strict '>' scan; status bits on the rounded values.
 * f16() is round to nearest even, past 65504 -> inf, written out bitwise (no _Float16 in this compiler).
 * The env (reset / observe / world step) is liboracle.so's: oracle_mpe_reset / _observe / _world_step.
 * Build: gcc -O2 -fPIC -shared -ffp-contract=off -mfma (the oracle's flags), linked against liboracle.so.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define H1 512
#define H2 256
#define NACT 5
#define LN_EPS 1e-5f

enum { ST_BAD_INPUT = 1, ST_BAD_FC1 = 2, ST_BAD_FC2 = 4, ST_BAD_OUT = 8, ST_NO_ACTION = 16 };

/* the oracle's env; the state is opaque here (a buffer larger than the oracle's mpe_state) */
typedef struct { double words[32]; } mpe_state_buf;
void oracle_mpe_reset(uint64_t st_hi, uint64_t st_lo, uint64_t inc_hi, uint64_t inc_lo, uint64_t ordinal, mpe_state_buf *s);
void oracle_mpe_observe(const mpe_state_buf *s, int slot, float *obs);
void oracle_mpe_world_step(mpe_state_buf *s, const int *act, double *r_good, double *r_adv);

uint16_t fc16_f32_to_f16(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
    if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (ax > 0x7f800000u ? 0x200u : 0u));   /* inf, NaN */
    if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);       /* >= 65520 rounds to inf */
    if (ax < 0x38800000u) {                                         /* below 2^-14: subnormal (or zero) half */
        float a;
        memcpy(&a, &ax, 4);
        return (uint16_t)(sign | (uint32_t)nearbyintf(a * 16777216.0f));   /* exact scaling, round to nearest even */
    }
    uint32_t h = ((((ax >> 23) - 127u + 15u) << 10) | ((ax & 0x7fffffu) >> 13));
    const uint32_t rem = ax & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h += 1u;     /* a carry into the exponent is the right result */
    return (uint16_t)(sign | h);
}

float fc16_f16_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t x;
    if (e == 0x1fu) x = sign | 0x7f800000u | (m << 13);
    else if (e == 0) {
        const float v = (float)m * (1.0f / 16777216.0f);            /* m * 2^-24, exact */
        memcpy(&x, &v, 4);
        x |= sign;
    } else x = sign | ((e - 15u + 127u) << 23) | (m << 13);
    float f;
    memcpy(&f, &x, 4);
    return f;
}

static float r16(float v) { return fc16_f16_to_f32(fc16_f32_to_f16(v)); }

static float block_tree64(const float *v)
{
    float t[64];
    memcpy(t, v, sizeof t);
    for (int w = 1; w < 64; w <<= 1)
        for (int i = 0; i < 64; i += 2 * w) t[i] = t[i] + t[i + w];
    return t[0];
}

static float reduce_canon(const float *v, int n)
{
    float s = block_tree64(v);
    for (int b = 1; b < n / 64; ++b) s = s + block_tree64(v + 64 * b);
    return s;
}

static int bad_post_relu(float y) { return isnan(y) || (isinf(y) && y > 0); }

static void layernorm16_relu(float *x, int n, const float *g, const float *be, int *bad)
{
    float tmp[H1];
    const float inv_n = 1.0f / (float)n;
    const float mean = reduce_canon(x, n) * inv_n;
    for (int j = 0; j < n; ++j) {
        const float d = x[j] - mean;
        x[j] = d;
        tmp[j] = d * d;
    }
    const float var = reduce_canon(tmp, n) * inv_n;
    const float rstd = 1.0f / sqrtf(var + LN_EPS);
    for (int j = 0; j < n; ++j) {
        const float y = r16(fmaf(x[j] * rstd, g[j], be[j]));
        if (bad_post_relu(y)) *bad = 1;
        x[j] = (y > 0.0f) ? y : (isnan(y) ? y : 0.0f);
    }
}

static void linear16(const float *W, const float *b, const float *x, float *y, int n_out, int n_in)
{
    for (int j = 0; j < n_out; ++j) {
        float acc = b[j];
        for (int k = 0; k < n_in; ++k) acc = fmaf(W[(size_t)j * n_in + k], x[k], acc);
        y[j] = r16(acc);
    }
}

/* p = the net in parameters() order as fp32 (Linear entries fp16 values, LayerNorm fp32) */
int fc16_forward(const float *p, int D, const float *obs, float *logits, int *status)
{
    const float *W1 = p, *b1 = W1 + H1 * D, *g1 = b1 + H1, *be1 = g1 + H1;
    const float *W2 = be1 + H1, *b2 = W2 + H2 * H1, *g2 = b2 + H2, *be2 = g2 + H2;
    const float *W3 = be2 + H2, *b3 = W3 + NACT * H2;
    float x[16], h1[H1], h2[H2];
    int st = 0, bad = 0;
    for (int k = 0; k < D; ++k) {
        x[k] = r16(obs[k]);
        if (!isfinite(x[k])) st |= ST_BAD_INPUT;
    }
    linear16(W1, b1, x, h1, H1, D);
    layernorm16_relu(h1, H1, g1, be1, &bad);
    if (bad) st |= ST_BAD_FC1;
    bad = 0;
    linear16(W2, b2, h1, h2, H2, H1);
    layernorm16_relu(h2, H2, g2, be2, &bad);
    if (bad) st |= ST_BAD_FC2;
    linear16(W3, b3, h2, logits, NACT, H2);
    int best = -1;
    float cur = -INFINITY;
    for (int i = 0; i < NACT; ++i) {
        if (!isfinite(logits[i])) st |= ST_BAD_OUT;
        if (logits[i] > cur) { cur = logits[i]; best = i; }
    }
    if (best < 0) st |= ST_NO_ACTION;
    if (status) *status |= st;
    return best;
}

/* oracle_play_game with the fp16 forward: nets by env slot (adversary_0, agent_0, agent_1); limit < 0 = None.
 * rewards_out in play_game's order (agent_0, agent_1, adversary_0); actions_out / margins_out one entry per agent-step. */
int fc16_play_game(const float *net_adv, const float *net_a0, const float *net_a1, uint64_t st_hi, uint64_t st_lo,
                   uint64_t inc_hi, uint64_t inc_lo, uint64_t ordinal, int limit, int max_cycles, double *rewards_out,
                   int *actions_out, float *margins_out, int *status_out)
{
    const float *nets[3] = {net_adv, net_a0, net_a1};
    static const int D[3] = {8, 10, 10};
    mpe_state_buf s;
    oracle_mpe_reset(st_hi, st_lo, inc_hi, inc_lo, ordinal, &s);
    double cum[3] = {0, 0, 0}, rew[3] = {0, 0, 0}, acc[3] = {0, 0, 0};
    int act[3] = {0, 0, 0};
    int sel = 0, world_steps = 0, trunc = 0, timesteps = 0, status = 0;
    for (;;) {
        const int agent = sel;
        float obs[10], logits[NACT];
        oracle_mpe_observe(&s, agent, obs);
        int a = fc16_forward(nets[agent], D[agent], obs, logits, &status);
        if (a < 0) a = 0;
        float top = -INFINITY, second = -INFINITY;
        for (int i = 0; i < NACT; ++i) {
            if (logits[i] > top) { second = top; top = logits[i]; }
            else if (logits[i] > second) second = logits[i];
        }
        if (actions_out) actions_out[timesteps] = a;
        if (margins_out) margins_out[timesteps] = top - second;
        const int cur = sel, nxt = (cur + 1) % 3;
        sel = nxt;
        act[cur] = a;
        if (nxt == 0) {
            double rg, ra;
            oracle_mpe_world_step(&s, act, &rg, &ra);
            rew[0] = ra; rew[1] = rg; rew[2] = rg;
            if (++world_steps >= max_cycles) trunc = 1;
        } else {
            rew[0] = rew[1] = rew[2] = 0.0;
        }
        cum[cur] = 0;
        for (int i = 0; i < 3; ++i) cum[i] += rew[i];
        acc[agent] += cum[sel];
        ++timesteps;
        if (limit >= 0 && timesteps >= limit) break;
        if (trunc) break;
    }
    rewards_out[0] = acc[1];
    rewards_out[1] = acc[2];
    rewards_out[2] = acc[0];
    if (status_out) *status_out = status;
    return timesteps;
}
