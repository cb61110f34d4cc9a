/*
 * dqn16_checker.c - TEST INFRASTRUCTURE ONLY: the float16 DeepQN forward restated in plain sequential C.
 *
 * The float16 contract (DESIGN.md 6a "Float16 DeepQN"; coevonet_amd/csrc/dqn16.hip reproduces it bit for bit):
 *   every parameter is an fp16 value (held here as fp32);
 *   x = f16(u8 / 255.0f): the IEEE fp32 quotient rounded once to fp16;
 *   conv: acc = bias, acc = fmaf(w, x, acc) over the taps in (ci, ky, kx) order in fp32, y = f16(acc);
 *   BatchNorm in training mode at batch 1: S = 64 lane-strided sums (lane l adds positions l, l + 64, ... left to right)
 *   combined by the adjacent-pairs tree, mean = S / N, d = y - mean, var = S(d * d) / N, rstd = 1 / sqrtf(var + 1e-5f),
 *   z = f16(fmaf(d * rstd, gamma, beta)); ReLU keeps NaN;
 *   fc1 / output: sequential-k fmaf chain from the bias in fp32, f16 of the sum; ReLU after fc1;
 *   action = first maximum of a strict '>' scan over the fp16 logits; ST_NO_ACTION when no logit compares (all NaN).
 * f16() is fc16_checker.c's bitwise rounding (round to nearest even, past 65504 -> inf, subnormals kept).
 * Flat order: conv1.w conv1.b conv2.w conv2.b conv3.w conv3.b fc1.w fc1.b output.w output.b vbn1.w vbn1.b vbn2.w vbn2.b
 * vbn3.w vbn3.b.  frame: uint8 [84][84][C].
 * Build: gcc -O2 -fPIC -shared -ffp-contract=off -fno-fast-math -mfma, together with fc16_checker.c.
 *
 * dqn16_forward_stages (below dqn16_forward, which it restates with no variant selected) returns every rounded stage and can
 * round WRONGLY at one of the nine conversion sites, or scan the logits wrongly: wrong kernels on paper, for
 * tests/test_dqn16_edges_cpu.py to show that a class of tests/dqn16_edge_nets.py would notice such a kernel.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define BN_EPS 1e-5f

enum { ST_NO_ACTION = 16 };

uint16_t fc16_f32_to_f16(float f);
float fc16_f16_to_f32(uint16_t h);

static float r16(float v) { return fc16_f16_to_f32(fc16_f32_to_f16(v)); }

static float relu_nan(float y) { return (y > 0.0f) ? y : (isnan(y) ? y : 0.0f); }

static float strided_sum(const float *v, int n)
{
    float lane[64];
    for (int l = 0; l < 64; ++l) {
        float s = (l < n) ? v[l] : 0.0f;
        for (int p = l + 64; p - l < ((n + 63) / 64) * 64; p += 64) s = s + ((p < n) ? v[p] : 0.0f);
        lane[l] = s;
    }
    for (int w = 1; w < 64; w <<= 1)
        for (int i = 0; i < 64; i += 2 * w) lane[i] = lane[i] + lane[i + w];
    return lane[0];
}

static void conv_bn_relu16(const float *in, int cin, int hin, const float *w, const float *b, const float *gamma,
                           const float *beta, int cout, int k, int stride, int hout, float *out)
{
    const int npos = hout * hout;
    float *sq = (float *)malloc(sizeof(float) * npos);
    for (int co = 0; co < cout; ++co) {
        float *o = out + (size_t)co * npos;
        for (int oy = 0; oy < hout; ++oy)
            for (int ox = 0; ox < hout; ++ox) {
                float acc = b[co];
                for (int ci = 0; ci < cin; ++ci)
                    for (int ky = 0; ky < k; ++ky)
                        for (int kx = 0; kx < k; ++kx)
                            acc = fmaf(w[(((size_t)co * cin + ci) * k + ky) * k + kx],
                                       in[((size_t)ci * hin + oy * stride + ky) * hin + ox * stride + kx], acc);
                o[oy * hout + ox] = r16(acc);
            }
        const float mean = strided_sum(o, npos) / (float)npos;
        for (int p = 0; p < npos; ++p) {
            o[p] = o[p] - mean;
            sq[p] = o[p] * o[p];
        }
        const float var = strided_sum(sq, npos) / (float)npos;
        const float rstd = 1.0f / sqrtf(var + BN_EPS);
        for (int p = 0; p < npos; ++p) o[p] = relu_nan(r16(fmaf(o[p] * rstd, gamma[co], beta[co])));
    }
    free(sq);
}

static void linear16(const float *W, const float *b, const float *x, float *y, int n_out, int n_in)
{
    for (int j = 0; j < n_out; ++j) {
        float acc = b[j];
        for (int k = 0; k < n_in; ++k) acc = fmaf(W[(size_t)j * n_in + k], x[k], acc);
        y[j] = r16(acc);
    }
}

/* -> the action (0 with ST_NO_ACTION when no logit compares, as the entry point stores it); logits[n] fp32 holding fp16
 * values; *status |= bits */
int dqn16_forward(const float *p, int C, int n, const unsigned char *frame, float *logits, int *status)
{
    const float *w1 = p, *b1 = w1 + 32 * C * 64, *w2 = b1 + 32, *b2 = w2 + 64 * 32 * 16, *w3 = b2 + 64,
                *b3 = w3 + 64 * 64 * 9, *wf = b3 + 64, *bf = wf + 512 * 3136, *wo = bf + 512, *bo = wo + 512 * n,
                *g1 = bo + n, *be1 = g1 + 32, *g2 = be1 + 32, *be2 = g2 + 64, *g3 = be2 + 64, *be3 = g3 + 64;
    float *x = (float *)malloc(sizeof(float) * C * 84 * 84);
    float *a1 = (float *)malloc(sizeof(float) * 32 * 400), *a2 = (float *)malloc(sizeof(float) * 64 * 81);
    float *a3 = (float *)malloc(sizeof(float) * 3136), *h = (float *)malloc(sizeof(float) * 512);
    for (int y = 0; y < 84; ++y)
        for (int xx = 0; xx < 84; ++xx)
            for (int c = 0; c < C; ++c)
                x[((size_t)c * 84 + y) * 84 + xx] = r16((float)frame[((size_t)y * 84 + xx) * C + c] / 255.0f);
    conv_bn_relu16(x, C, 84, w1, b1, g1, be1, 32, 8, 4, 20, a1);
    conv_bn_relu16(a1, 32, 20, w2, b2, g2, be2, 64, 4, 2, 9, a2);
    conv_bn_relu16(a2, 64, 9, w3, b3, g3, be3, 64, 3, 1, 7, a3);
    linear16(wf, bf, a3, h, 512, 3136);
    for (int j = 0; j < 512; ++j) h[j] = relu_nan(h[j]);
    linear16(wo, bo, h, logits, n, 512);
    int best = -1;
    float cur = -INFINITY;
    for (int i = 0; i < n; ++i)
        if (logits[i] > cur) { cur = logits[i]; best = i; }
    if (best < 0) {
        if (status) *status |= ST_NO_ACTION;
        best = 0;
    }
    free(x); free(a1); free(a2); free(a3); free(h);
    return best;
}

/* ------------------------------------------------------------------------------------------------ stages and variants */
enum { SITE_NONE = -1, SITE_QUOTIENT, SITE_CONV1, SITE_BN1, SITE_CONV2, SITE_BN2, SITE_CONV3, SITE_BN3, SITE_FC1, SITE_OUT };
enum { MODE_NEAREST_EVEN, MODE_TOWARD_ZERO, MODE_TIES_AWAY, MODE_FLUSH_RESULTS, MODE_SATURATE };
enum { ACT_FIRST_MAXIMUM, ACT_SCAN_BEFORE_ROUNDING, ACT_LAST_MAXIMUM };

/* fp32 -> fp16 under `mode`, as fp32.  nearest_even is f16() of the contract; the others are what a wrong conversion does:
 * toward_zero truncates (a finite value never reaches inf), ties_away takes an exact midpoint away from zero, flush_results
 * turns a rounded result below 2^-14 into a zero of its sign, saturate returns +-65504 where a finite value rounds to inf */
static float rmode(float v, int mode)
{
    uint16_t h = fc16_f32_to_f16(v);
    const float r = fc16_f16_to_f32(h);
    if (mode == MODE_NEAREST_EVEN || isnan(v)) return r;
    if (mode == MODE_TOWARD_ZERO) {
        if (fabsf(r) > fabsf(v)) h -= 1;   /* the magnitude bits: inf -> 65504, 2^-24 -> 0 */
    } else if (mode == MODE_TIES_AWAY) {
        if (fabsf(r) < fabsf(v)) {
            const uint16_t up = (uint16_t)(h + 1);
            const double above = ((up & 0x7fff) == 0x7c00) ? 65536.0 : fabs((double)fc16_f16_to_f32(up));
            if (fabs((double)v) == (fabs((double)r) + above) / 2) h = up;
        }
    } else if (mode == MODE_FLUSH_RESULTS) {
        if (fabsf(r) < 6.103515625e-05f) h &= 0x8000;
    } else if (mode == MODE_SATURATE) {
        if (isinf(r) && !isinf(v)) h -= 1;
    }
    return fc16_f16_to_f32(h);
}

float dqn16_round_mode(float v, int mode) { return rmode(v, mode); }

static int mode_at(int site, int here, int mode) { return site == here ? mode : MODE_NEAREST_EVEN; }

/* conv_bn_relu16 with the rounded conv sums kept in `sums` and the two conversions under their own modes */
static void conv_bn_relu16_stages(const float *in, int cin, int hin, const float *w, const float *b, const float *gamma,
                                  const float *beta, int cout, int k, int stride, int hout, float *sums, float *out,
                                  int mode_conv, int mode_bn)
{
    const int npos = hout * hout;
    float *sq = (float *)malloc(sizeof(float) * npos);
    for (int co = 0; co < cout; ++co) {
        float *y = sums + (size_t)co * npos, *o = out + (size_t)co * npos;
        for (int oy = 0; oy < hout; ++oy)
            for (int ox = 0; ox < hout; ++ox) {
                float acc = b[co];
                for (int ci = 0; ci < cin; ++ci)
                    for (int ky = 0; ky < k; ++ky)
                        for (int kx = 0; kx < k; ++kx)
                            acc = fmaf(w[(((size_t)co * cin + ci) * k + ky) * k + kx],
                                       in[((size_t)ci * hin + oy * stride + ky) * hin + ox * stride + kx], acc);
                y[oy * hout + ox] = rmode(acc, mode_conv);
            }
        const float mean = strided_sum(y, npos) / (float)npos;
        for (int p = 0; p < npos; ++p) {
            o[p] = y[p] - mean;
            sq[p] = o[p] * o[p];
        }
        const float var = strided_sum(sq, npos) / (float)npos;
        const float rstd = 1.0f / sqrtf(var + BN_EPS);
        for (int p = 0; p < npos; ++p) o[p] = relu_nan(rmode(fmaf(o[p] * rstd, gamma[co], beta[co]), mode_bn));
    }
    free(sq);
}

/* the forward with its stages: x [C][84][84] (the quotient image), s1 / a1 [32][400], s2 / a2 [64][81], s3 / a3 [64][49] (rounded
 * conv sums / BatchNorm + ReLU outputs), hid [512] (after ReLU), logits [n]; -> the action, *status |= bits, as dqn16_forward.
 * site (SITE_NONE: none) rounds under `mode`; `action_variant` scans the fp32 sums in front of the output conversion, or takes
 * the last maximum (a '>=' scan). */
int dqn16_forward_stages(const float *p, int C, int n, const unsigned char *frame, int site, int mode, int action_variant,
                         float *x, float *s1, float *a1, float *s2, float *a2, float *s3, float *a3, float *hid, float *logits,
                         int *status)
{
    const float *w1 = p, *b1 = w1 + 32 * C * 64, *w2 = b1 + 32, *b2 = w2 + 64 * 32 * 16, *w3 = b2 + 64,
                *b3 = w3 + 64 * 64 * 9, *wf = b3 + 64, *bf = wf + 512 * 3136, *wo = bf + 512, *bo = wo + 512 * n,
                *g1 = bo + n, *be1 = g1 + 32, *g2 = be1 + 32, *be2 = g2 + 64, *g3 = be2 + 64, *be3 = g3 + 64;
    float sums[32];
    if (n > 32) return -2;
    for (int y = 0; y < 84; ++y)
        for (int xx = 0; xx < 84; ++xx)
            for (int c = 0; c < C; ++c)
                x[((size_t)c * 84 + y) * 84 + xx] =
                    rmode((float)frame[((size_t)y * 84 + xx) * C + c] / 255.0f, mode_at(site, SITE_QUOTIENT, mode));
    conv_bn_relu16_stages(x, C, 84, w1, b1, g1, be1, 32, 8, 4, 20, s1, a1, mode_at(site, SITE_CONV1, mode),
                          mode_at(site, SITE_BN1, mode));
    conv_bn_relu16_stages(a1, 32, 20, w2, b2, g2, be2, 64, 4, 2, 9, s2, a2, mode_at(site, SITE_CONV2, mode),
                          mode_at(site, SITE_BN2, mode));
    conv_bn_relu16_stages(a2, 64, 9, w3, b3, g3, be3, 64, 3, 1, 7, s3, a3, mode_at(site, SITE_CONV3, mode),
                          mode_at(site, SITE_BN3, mode));
    for (int j = 0; j < 512; ++j) {
        float acc = bf[j];
        for (int k = 0; k < 3136; ++k) acc = fmaf(wf[(size_t)j * 3136 + k], a3[k], acc);
        hid[j] = relu_nan(rmode(acc, mode_at(site, SITE_FC1, mode)));
    }
    for (int j = 0; j < n; ++j) {
        float acc = bo[j];
        for (int k = 0; k < 512; ++k) acc = fmaf(wo[(size_t)j * 512 + k], hid[k], acc);
        sums[j] = acc;
        logits[j] = rmode(acc, mode_at(site, SITE_OUT, mode));
    }
    const float *scan = (action_variant == ACT_SCAN_BEFORE_ROUNDING) ? sums : logits;
    int best = -1;
    float cur = -INFINITY;
    for (int i = 0; i < n; ++i)
        if (action_variant == ACT_LAST_MAXIMUM ? scan[i] >= cur : scan[i] > cur) { cur = scan[i]; best = i; }
    if (best < 0) {
        if (status) *status |= ST_NO_ACTION;
        best = 0;
    }
    return best;
}
