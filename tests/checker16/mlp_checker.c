/*
 * mlp_checker.c - TEST INFRASTRUCTURE ONLY: the PPO policy net of a baseline seat (D -> 64 -> 64 -> 5, ReLU) restated in plain
 * sequential C with a real fmaf (a float64 emulation would round twice).
 *
 * The contract (include/coevo_baseline.h; coevonet_amd/csrc/baseline.hip reproduces it bit for bit): flat order fc1.weight
 * [64][D], fc1.bias, fc2.weight [64][64], fc2.bias, policy_head.weight [5][64], policy_head.bias; every output one fmaf chain
 * over k ascending that starts from the bias; ReLU v > 0 ? v : +0; first maximum by a strict '>' scan; a non-finite observation,
 * fc1 output, fc2 output (both before the ReLU) or logit raises its status bit and the row plays 0.
 * Build: gcc -O2 -fPIC -shared -ffp-contract=off -fno-fast-math -mfma.
 */
#include <math.h>

#define H 64
#define NACT 5

enum { ST_BAD_INPUT = 1, ST_BAD_FC1 = 2, ST_BAD_FC2 = 4, ST_BAD_OUT = 8 };

static float relu(float v) { return v > 0.0f ? v : 0.0f; }

/* -> the action; logits [5] as computed, *status = the bits of this row */
int mlp_forward(const float *p, int D, const float *obs, float *logits, int *status)
{
    const float *W1 = p, *b1 = W1 + H * D, *W2 = b1 + H, *b2 = W2 + H * H, *W3 = b2 + H, *b3 = W3 + NACT * H;
    float h1[H], h2[H];
    int st = 0;
    for (int k = 0; k < D; ++k)
        if (!isfinite(obs[k])) st |= ST_BAD_INPUT;
    for (int j = 0; j < H; ++j) {
        float a = b1[j];
        for (int k = 0; k < D; ++k) a = fmaf(W1[j * D + k], obs[k], a);
        if (!isfinite(a)) st |= ST_BAD_FC1;
        h1[j] = relu(a);
    }
    for (int j = 0; j < H; ++j) {
        float a = b2[j];
        for (int k = 0; k < H; ++k) a = fmaf(W2[j * H + k], h1[k], a);
        if (!isfinite(a)) st |= ST_BAD_FC2;
        h2[j] = relu(a);
    }
    for (int c = 0; c < NACT; ++c) {
        float a = b3[c];
        for (int k = 0; k < H; ++k) a = fmaf(W3[c * H + k], h2[k], a);
        if (!isfinite(a)) st |= ST_BAD_OUT;
        logits[c] = a;
    }
    *status = st;
    if (st) return 0;
    int best = 0;
    float cur = logits[0];
    for (int c = 1; c < NACT; ++c)
        if (logits[c] > cur) { cur = logits[c]; best = c; }
    return best;
}

/* n rows of obs [n][obs_stride] -> actions [n], logits [n][5], the OR of the rows' status bits */
int mlp_forward_rows(const float *p, int D, const float *obs, int obs_stride, int n, int *actions, float *logits, int *row_status)
{
    int all = 0;
    for (int i = 0; i < n; ++i) {
        int st = 0;
        actions[i] = mlp_forward(p, D, obs + (long)i * obs_stride, logits + (long)i * NACT, &st);
        if (row_status) row_status[i] = st;
        all |= st;
    }
    return all;
}
