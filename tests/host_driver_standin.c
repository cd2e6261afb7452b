/* tests/host_driver_standin.c — TEST INFRASTRUCTURE, never shipped or linked into libencoder.so.
 *
 * A CPU stand-in for the handful of m1v_* entry points that csrc/encoder_host.c calls, implemented with
 * the oracle (oracle/mpeg1_oracle.c).  tests/test_host_driver_cpu.py links it with encoder_host.c under
 * -fsanitize=thread / address so that the host driver's own logic — directory scan order, parallel
 * decode, batch staging, global frame indices across batches, .bit write-behind, error returns — runs
 * in this GPU-less container against the real reference binary's output.  It says nothing about the
 * HIP kernels; those are checked on the GPU box through the real library.
 *
 * Failure knobs (tests/test_host_driver_faults_cpu.py).  Each is an environment variable that holds a comma-separated
 * list of call numbers, read at EVERY call (a test program may change it between two calls of the driver); the calls of
 * a kind are counted per process with an atomic counter, from 1, because the driver's lanes run on pool threads.
 * Unset or empty = the call behaves as ever.
 *   STANDIN_FAIL_CREATE=k[,k..]     the k-th m1v_create returns M1V_E_HIP and leaves *out NULL
 *   STANDIN_FAIL_ALLOC=k[,k..]      the k-th m1v_alloc_host returns NULL
 *   STANDIN_FAIL_ENCODE=k[,k..]     the k-th m1v_encode_planes_host returns M1V_E_HIP and writes nothing
 *   STANDIN_NOSPACE_ENCODE=k[,k..]  the k-th m1v_encode_planes_host returns M1V_E_NOSPACE whatever the capacity
 * A failing call leaves "injected failure (<knob> <k>)" in m1v_last_error() of its thread (per thread, as in the library).
 * standin_counts() reads the three counters, standin_reset_counts() sets them back to 0.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mpeg1_hip.h"
#include "mpeg1_oracle.h"

struct m1v_encoder {
    int W, H, C, qf, mode, max_frames;
};

static _Thread_local const char *g_err = "";
static _Thread_local char g_err_buf[96];
static int g_calls[3]; /* m1v_create, m1v_alloc_host, m1v_encode_planes_host */

void standin_counts(int out[3]) {
    for (int i = 0; i < 3; i++) out[i] = __atomic_load_n(&g_calls[i], __ATOMIC_SEQ_CST);
}

void standin_reset_counts(void) {
    for (int i = 0; i < 3; i++) __atomic_store_n(&g_calls[i], 0, __ATOMIC_SEQ_CST);
}

/* is call number k in the list that the knob holds right now? */
static int knob_names(const char *knob, int k) {
    const char *v = getenv(knob);
    while (v && *v) {
        char *end;
        long x = strtol(v, &end, 10);
        if (end == v) break;
        if (x == k) {
            snprintf(g_err_buf, sizeof g_err_buf, "injected failure (%s %d)", knob, k);
            g_err = g_err_buf;
            return 1;
        }
        v = *end == ',' ? end + 1 : end;
    }
    return 0;
}

const char *m1v_last_error(void) { return g_err; }
int m1v_warm_up(int device) { (void)device; return M1V_OK; }
size_t m1v_file_prolog(uint8_t out[27]) { return orc_file_prolog(out); }

int m1v_create(m1v_encoder **out, int device, int w, int h, int channels, int qf, int mode, int max_frames) {
    (void)device;
    int xe, ye;
    *out = NULL;
    if (knob_names("STANDIN_FAIL_CREATE", __atomic_add_fetch(&g_calls[0], 1, __ATOMIC_SEQ_CST))) return M1V_E_HIP;
    orc_region(mode == M1V_MODE_FULL ? ORC_MODE_FULL : ORC_MODE_STRICT, w, h, &xe, &ye);
    if (xe > w || ye > h || channels < 3) {
        g_err = "picture smaller than the encoded region";
        return M1V_E_ARG;
    }
    m1v_encoder *e = (m1v_encoder *)calloc(1, sizeof *e);
    e->W = w, e->H = h, e->C = channels, e->qf = qf, e->max_frames = max_frames;
    e->mode = mode == M1V_MODE_FULL ? ORC_MODE_FULL : ORC_MODE_STRICT;
    *out = e;
    return M1V_OK;
}
void m1v_destroy(m1v_encoder *e) { free(e); }
size_t m1v_frame_bytes_in(const m1v_encoder *e) { return (size_t)e->W * e->H * e->C; }
size_t m1v_frame_bound(const m1v_encoder *e) { return orc_frame_bound(e->W, e->H, e->mode); }
size_t m1v_frame_bound_for(int width, int height, int mode) { return orc_frame_bound(width, height, mode); }
void *m1v_alloc_host(size_t bytes) {
    if (knob_names("STANDIN_FAIL_ALLOC", __atomic_add_fetch(&g_calls[1], 1, __ATOMIC_SEQ_CST))) return NULL;
    return malloc(bytes ? bytes : 1);
}
void m1v_free_host(void *p) { free(p); }

long m1v_encode_planes_host(m1v_encoder *e, const uint8_t *rgb, int n, int first, uint8_t *out, size_t cap,
                            uint64_t *sizes, uint8_t *planes) {
    const int k = __atomic_add_fetch(&g_calls[2], 1, __ATOMIC_SEQ_CST);
    if (knob_names("STANDIN_FAIL_ENCODE", k)) return M1V_E_HIP;
    if (knob_names("STANDIN_NOSPACE_ENCODE", k)) return M1V_E_NOSPACE;
    if (n > e->max_frames) {
        g_err = "n_frames exceeds max_frames";
        return M1V_E_ARG;
    }
    long r = orc_encode_frames(rgb, n, e->W, e->H, e->C, first, e->qf, e->mode, 1, out, cap, sizes);
    if (r == ORC_E_UNENCODABLE) return M1V_E_UNENCODABLE;
    if (r == ORC_E_NOSPACE) {
        g_err = "output buffer too small";
        return M1V_E_NOSPACE;
    }
    if (r < 0) return M1V_E_ARG;
    size_t npx = (size_t)e->W * e->H;
    for (int f = 0; planes && f < n; f++) {
        uint8_t *p = planes + 3 * npx * (size_t)f;
        orc_convert_rgb_to_ycbcr(rgb + npx * e->C * (size_t)f, e->C, npx, p, p + npx, p + 2 * npx);
    }
    return r;
}
