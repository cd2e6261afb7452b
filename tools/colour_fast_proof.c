/* tools/colour_fast_proof.c — exhaustive host-side proof of the kernel's fp32 colour fast path
 * (m1v_kernels.hip: component_t / clear_fraction / convert_row).  For every (r,g,b) and each of Y, Cb, Cr:
 *     t    = fmaf(r, kr, fmaf(g, kg, fmaf(b, kb, k0 + 256 + eps)))          (same order, same constants)
 *     p    = t with its low 15 mantissa bits cleared (= 256 + trunc(t - 256));   d = t - p  (exact)
 * a pixel is "flagged" (redone in fp64 by the kernel) when d < LOW; for every unflagged pixel p - 256 must equal the
 * reference's fp64, unfused, left-to-right value truncated to int (image_processing.c:104-106), and t must lie in
 * [256, 512) for EVERY pixel (the bit trick assumes that exponent).
 *     gcc -O2 -ffp-contract=off -frounding-math tools/colour_fast_proof.c -o build/colour_fast_proof -lm && build/colour_fast_proof [down]
 *
 * "denormal" (with or without "down"): the luma row of the tile kernels (luma_sums_denormal) takes a colour byte where it lies in
 * its dword, masked in place and read as a float — b * 2^(8q - 149), a denormal, for byte position q = 0, 1, 2, and w >> 24 at
 * the scale of q = 0 for q = 3 — and multiplies it by fl32(k_c) * 2^(125 - 8q), starting from fl32(k0 + 256 + eps) * 2^-24.
 * Every product is the same real number * 2^-24 and every sum stays normal (>= 2^-16), so each fma rounds where the unit-scale
 * one does.  For every (r,g,b), Y, and each of the four dword phases a pixel can start at, checked here:
 *     t' == t * 2^-24 bit for bit (same mantissa, exponent 24 lower);
 *     the low 15 mantissa bits of t' as an integer, L, satisfy  L < 10  exactly when  t - p < LOW  (the same pixels flagged);
 *     (bits(t') & 0x007f8000) | bits(256.0f) == bits(p)  (the raw pixel at unit scale from one and-or).
 * The host must not flush denormals (no -ffast-math: checked at start).
 */
#include <fenv.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define EPS 1.5e-4f
#define LOW (10.0f / 32768.0f) /* kFracLow */

static float as_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t as_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

/* the denormal form of the Y sum against the unit-scale form: see the head of the file */
static int denormal_mode(int down) {
    const float kf[3] = {0.299f, 0.587f, 0.114f}; /* r, g, b */
    const float k0 = 0.0f + 256.0f + EPS, k0s = ldexpf(k0, -24);
    float ks[3][4]; /* coefficient of channel c for a byte at position q */
    volatile float tiny = as_float(1u);
    if (tiny * 1.0f == 0.0f || as_bits(tiny * 2.0f) != 2u) {
        printf("the host flushes denormals\n");
        return 2;
    }
    for (int c = 0; c < 3; c++)
        for (int q = 0; q < 4; q++) ks[c][q] = ldexpf(kf[c], 125 - 8 * (q == 3 ? 0 : q));
    long long differ = 0, flags_differ = 0, pixel_differ = 0, subnormal = 0, flagged = 0;
    if (down) fesetround(FE_DOWNWARD);
    for (int phase = 0; phase < 4; phase++) /* the pixel's first byte is byte `phase` of a dword */
        for (int r = 0; r < 256; r++)
            for (int g = 0; g < 256; g++)
                for (int b = 0; b < 256; b++) {
                    const int ch[3] = {r, g, b};
                    volatile float x[3];
                    int q[3];
                    for (int c = 0; c < 3; c++) { /* the dword holds other pixels' bytes around this one: all ones */
                        q[c] = (phase + c) & 3;
                        const uint32_t w = (0xffffffffu & ~(0xffu << (8 * q[c]))) | ((uint32_t)ch[c] << (8 * q[c]));
                        x[c] = as_float(q[c] == 3 ? w >> 24 : w & (0xffu << (8 * q[c])));
                    }
                    volatile float t = fmaf((float)b, kf[2], k0);
                    t = fmaf((float)g, kf[1], t);
                    t = fmaf((float)r, kf[0], t);
                    volatile float u = fmaf(x[2], ks[2][q[2]], k0s);
                    u = fmaf(x[1], ks[1][q[1]], u);
                    u = fmaf(x[0], ks[0][q[0]], u);
                    const uint32_t tb = as_bits(t), ub = as_bits(u);
                    if (ub + (24u << 23) != tb) {
                        if (differ < 10) printf("DIFFER phase %d rgb %d %d %d: t=%a t'=%a\n", phase, r, g, b, t, u);
                        differ++;
                    }
                    if ((ub >> 23) == 0) subnormal++;
                    const float p = as_float(tb & 0xffff8000u);
                    const int flag = t - p < LOW, flag_s = (ub & 0x7fffu) < 10u;
                    flagged += flag;
                    if (flag != flag_s) flags_differ++;
                    if (((ub & 0x007f8000u) | as_bits(256.0f)) != as_bits(p)) pixel_differ++;
                }
    fesetround(FE_TONEAREST);
    printf("denormal%s: 4 phases x 16777216 triples; flagged %lld per phase; t' != t * 2^-24: %lld; flags differ: %lld; "
           "pixels differ: %lld; subnormal sums: %lld\n",
           down ? " down" : "", flagged / 4, differ, flags_differ, pixel_differ, subnormal);
    return differ != 0 || flags_differ != 0 || pixel_differ != 0 || subnormal != 0;
}

int main(int argc, char **argv) {
    /* "down": the three fmas rounded toward minus infinity (the encode kernels' pixel stage runs in that mode, fdct_f32.h);
     * the reference's fp64 expression stays in round-to-nearest */
    int down = 0, denormal = 0;
    for (int i = 1; i < argc; i++) {
        down |= strcmp(argv[i], "down") == 0;
        denormal |= strcmp(argv[i], "denormal") == 0;
    }
    if (denormal) return denormal_mode(down);
    const double k0d[3] = {0.0, 128.0, 128.0};
    const double krd[3] = {0.299, -0.168736, 0.5}, kgd[3] = {0.587, -0.331264, -0.418688}, kbd[3] = {0.114, 0.5, -0.081312};
    const float krf[3] = {0.299f, -0.168736f, 0.5f}, kgf[3] = {0.587f, -0.331264f, -0.418688f},
                kbf[3] = {0.114f, 0.5f, -0.081312f};
    long long flagged[3] = {0, 0, 0}, wrong = 0, outside = 0;
    for (int c = 0; c < 3; c++) {
        const float k0 = (float)k0d[c] + 256.0f + EPS;
        for (int r = 0; r < 256; r++)
            for (int g = 0; g < 256; g++)
                for (int b = 0; b < 256; b++) {
                    volatile double acc = k0d[c] + krd[c] * (double)r;
                    acc = acc + kgd[c] * (double)g;
                    acc = acc + kbd[c] * (double)b;
                    int want = (int)acc;
                    if (down) fesetround(FE_DOWNWARD);
                    volatile float t = fmaf((float)b, kbf[c], k0);
                    t = fmaf((float)g, kgf[c], t);
                    t = fmaf((float)r, krf[c], t);
                    if (down) fesetround(FE_TONEAREST);
                    uint32_t bits;
                    { float tt = t; memcpy(&bits, &tt, 4); }
                    bits &= 0xffff8000u;
                    float p;
                    memcpy(&p, &bits, 4);
                    if (t < 256.0f || t >= 512.0f) outside++;
                    if (t - p < LOW) {
                        flagged[c]++;
                        continue;
                    }
                    if ((int)(p - 256.0f) != want) {
                        if (wrong < 10)
                            printf("WRONG comp %d rgb %d %d %d: t=%.9g p-256=%d want %d\n", c, r, g, b, t, (int)(p - 256.0f), want);
                        wrong++;
                    }
                }
    }
    printf("flagged: Y %lld  Cb %lld  Cr %lld of 16777216 each; t outside [256, 512): %lld; wrong: %lld\n",
           flagged[0], flagged[1], flagged[2], outside, wrong);
    return wrong != 0 || outside != 0;
}
