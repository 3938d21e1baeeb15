#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dm3d.h"
/* host-side paths of dm3d_grad_scale, dm3d_adam_scaled and dm3d_adam_ema with hostile arguments (no device needed: each must refuse before any launch).
 * The buffers are real heap blocks of exactly the documented sizes, so a host-side read or write past them is a sanitizer report. */
static int refused(int rc, const char* entry) {
    return rc == DM3D_EINVAL && strstr(dm3d_last_error(), entry) != NULL;
}
int main(void) {
    int bad = 0, total = 0;
    const int64_t n = 64;
    float* buf[5];                                           /* w, g, m, v, ema */
    for (int i = 0; i < 5; ++i) buf[i] = (float*)aligned_alloc(64, (size_t)n * sizeof(float));
    double* parts = (double*)aligned_alloc(64, DM3D_GRADNORM_PARTIAL_BLOCKS * sizeof(double));
    float* state = (float*)aligned_alloc(64, 64);
    dm3d_gradscale_desc ok;
    memset(&ok, 0, sizeof ok);
    ok.g = buf[1]; ok.n = n; ok.partials = parts; ok.state = state; ok.clip_norm = 1.0f; ok.pre_scale = 1.0f;
    dm3d_gradscale_desc d;
#define GS(change) do { d = ok; change; ++total; bad += refused(dm3d_grad_scale(&d, NULL), "grad_scale"); } while (0)
    ++total; bad += refused(dm3d_grad_scale(NULL, NULL), "grad_scale");
    GS(d.g = NULL); GS(d.partials = NULL); GS(d.state = NULL);
    GS(d.g = (const float*)((const char*)buf[1] + 4)); GS(d.partials = (double*)((char*)parts + 4)); GS(d.state = (float*)((char*)state + 4));
    GS(d.n = 0); GS(d.n = 6); GS(d.n = -4);
    GS(d.clip_norm = 0.0f); GS(d.clip_norm = -1.0f); GS(d.clip_norm = NAN);
    GS(d.pre_scale = 0.0f); GS(d.pre_scale = -1.0f); GS(d.pre_scale = NAN); GS(d.pre_scale = INFINITY);
#define AS(w, g, m, v, e, cnt, rate, st) do { ++total; \
    bad += refused(dm3d_adam_scaled(w, g, m, v, e, cnt, 1e-4f, 0.9f, 0.999f, 1e-7f, rate, st, NULL), "adam_scaled"); } while (0)
    float *w = buf[0], *g = buf[1], *m = buf[2], *v = buf[3], *e = buf[4];
    AS(NULL, g, m, v, e, n, 0.1f, state); AS(w, NULL, m, v, e, n, 0.1f, state); AS(w, g, NULL, v, e, n, 0.1f, state);
    AS(w, g, m, NULL, e, n, 0.1f, state); AS(w, g, m, v, e, n, 0.1f, NULL);
    AS(w + 1, g, m, v, e, n, 0.1f, state); AS(w, g + 1, m, v, e, n, 0.1f, state); AS(w, g, m + 1, v, e, n, 0.1f, state);
    AS(w, g, m, v + 1, e, n, 0.1f, state); AS(w, g, m, v, e + 1, n, 0.1f, state); AS(w, g, m, v, e, n, 0.1f, state + 1);
    AS(w, g, m, v, e, 0, 0.1f, state); AS(w, g, m, v, e, 6, 0.1f, state); AS(w, g, m, v, e, -4, 0.1f, state);
    AS(w, g, m, v, e, n, -0.1f, state); AS(w, g, m, v, e, n, 1.5f, state); AS(w, g, m, v, e, n, NAN, state);
    AS(w, g, m, v, w, n, 0.1f, state); AS(w, g, m, v, g, n, 0.1f, state); AS(w, g, m, v, m, n, 0.1f, state);
    AS(w, g, m, v, v, n, 0.1f, state); AS(w, g, m, v, w + 4, n, 0.1f, state);
    AS(w, g, m, v, e, n, 0.1f, w + 8); AS(w, g, m, v, e, n, 0.1f, m); AS(w, g, m, v, e, n, 0.1f, v + 60); AS(w, g, m, v, e, n, 0.1f, e + 4);
    AS(w, g, m, v, NULL, 6, 0.1f, state);                    /* ema = NULL passes the pointer checks: n is what is refused */
    /* dm3d_adam_ema: the same table through the other door of the validator the two entries share */
#define AE(w, g, m, v, e, cnt, rate) do { ++total; \
    bad += refused(dm3d_adam_ema(w, g, m, v, e, cnt, 1e-4f, 0.9f, 0.999f, 1e-7f, rate, NULL), "adam_ema"); } while (0)
    AE(NULL, g, m, v, e, n, 0.1f); AE(w, NULL, m, v, e, n, 0.1f); AE(w, g, NULL, v, e, n, 0.1f); AE(w, g, m, NULL, e, n, 0.1f);
    AE(w, g, m, v, NULL, n, 0.1f);
    AE(w + 1, g, m, v, e, n, 0.1f); AE(w, g + 1, m, v, e, n, 0.1f); AE(w, g, m + 1, v, e, n, 0.1f); AE(w, g, m, v + 1, e, n, 0.1f);
    AE(w, g, m, v, e + 1, n, 0.1f);
    AE(w, g, m, v, e, 0, 0.1f); AE(w, g, m, v, e, 6, 0.1f); AE(w, g, m, v, e, -4, 0.1f);
    AE(w, g, m, v, e, n, -0.1f); AE(w, g, m, v, e, n, 1.5f); AE(w, g, m, v, e, n, NAN);
    AE(w, g, m, v, w, n, 0.1f); AE(w, g, m, v, g, n, 0.1f); AE(w, g, m, v, m, n, 0.1f); AE(w, g, m, v, v, n, 0.1f);
    AE(w, g, m, v, w + 4, n, 0.1f); AE(w, g, m, v, g + 60, n, 0.1f); AE(w, g, m, v, m + 32, n, 0.1f); AE(w, g, m, v, v + 8, n, 0.1f);
    printf("refused %d of %d; last error: %s\n", bad, total, dm3d_last_error());
    for (int i = 0; i < 5; ++i) free(buf[i]);
    free(parts); free(state);
    return bad == total ? 0 : 1;
}
