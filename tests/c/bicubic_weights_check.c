/*
 * vp9hip_bicubic_weights (csrc/host/vp9h_convert.c) at the extreme sizes, where T = 2^15 and
 * c 2^Q nears 2^61: every weight against a 128-bit evaluation of the formulas of
 * include/vp9hip.h, the sums, the footprint's ends and the argument errors. Stand-alone (its
 * own main, no device); `make sanitize` builds it plain and with ASan + UBSan, and the weights
 * go into exact-size heap arrays, so an overflow of either kind is reported.
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/vp9hip.h"

#define Q 14
static long checked;

/* q from the definition, in 128 bits; -1 << 20 if the tap is absent */
static int64_t ref_q(int n_src, int n_out, int o, int64_t s)
{
    const __int128 t = 2 * (__int128) (n_src > n_out ? n_src : n_out);
    __int128 u = (2 * (__int128) o + 1) * n_src - (2 * (__int128) s + 1) * n_out;
    if (u < 0) u = -u;
    if (u >= 2 * t) return -(1 << 20);
    const __int128 t3 = t * t * t;
    const __int128 c = u < t ? 3 * u * u * u - 5 * t * u * u + 2 * t3 : -u * u * u + 5 * t * u * u - 8 * t * t * u + 4 * t3;
    const __int128 num = c * ((__int128) 1 << Q) + t3, den = 2 * t3;
    __int128 q = num / den;
    if (num % den < 0) q--;
    return (int64_t) q;
}

static int check_row(int n_src, int n_out, int o)
{
    int first = -1;
    int64_t sum = 0, abs_sum = 0;
    const int n = vp9hip_bicubic_weights(n_src, n_out, o, &first, NULL, 0, &sum, &abs_sum);
    if (n < 1 || first < 0 || first + n > n_src) {
        printf("%d -> %d, o %d: %d taps from %d\n", n_src, n_out, o, n, first);
        return 1;
    }
    int32_t *w = malloc((size_t) n * sizeof(*w));        /* exact size: a tap too many is a heap overflow */
    if (!w) return 1;
    int bad = vp9hip_bicubic_weights(n_src, n_out, o, NULL, w, n, NULL, NULL) != n;
    int64_t d = 0, a = 0;
    for (int i = 0; i < n && !bad; i++) {
        const int64_t q = ref_q(n_src, n_out, o, first + i);
        if (q != w[i] || q > (1 << Q) || q < -1214) {
            printf("%d -> %d, o %d, s %d: %d, the definition has %lld\n", n_src, n_out, o, first + i, w[i], (long long) q);
            bad = 1;
        }
        d += q;
        a += q < 0 ? -q : q;
    }
    free(w);
    if (bad) return 1;
    if (d != sum || a != abs_sum || d <= 0) {
        printf("%d -> %d, o %d: sums %lld %lld, the definition has %lld %lld\n", n_src, n_out, o, (long long) sum,
               (long long) abs_sum, (long long) d, (long long) a);
        return 1;
    }
    /* the taps on either side are absent */
    if ((first > 0 && ref_q(n_src, n_out, o, first - 1) != -(1 << 20)) ||
        (first + n < n_src && ref_q(n_src, n_out, o, first + n) != -(1 << 20))) {
        printf("%d -> %d, o %d: a present tap outside [%d, %d)\n", n_src, n_out, o, first, first + n);
        return 1;
    }
    checked += n;
    return 0;
}

int main(void)
{
    /* (n_src, n_out, step over o): T = 2^15 from either side, odd neighbours, the flagship ratios */
    static const int sweep[][3] = { { 16384, 1, 1 }, { 16384, 2, 1 }, { 16384, 3, 1 }, { 16384, 16384, 97 }, { 16384, 16383, 89 },
                                    { 16383, 16384, 83 }, { 1, 16384, 61 }, { 2, 16384, 67 }, { 16384, 4097, 31 },
                                    { 4099, 16384, 71 }, { 7680, 224, 1 }, { 4320, 224, 1 }, { 16384, 224, 5 }, { 5, 3, 1 } };
    for (unsigned i = 0; i < sizeof(sweep) / sizeof(sweep[0]); i++) {
        const int n_src = sweep[i][0], n_out = sweep[i][1];
        for (int o = 0; o < n_out; o += sweep[i][2])
            if (check_row(n_src, n_out, o)) return 1;
        if (check_row(n_src, n_out, n_out - 1)) return 1;
    }
    /* the argument errors; a cap below the count leaves the rest of the array alone */
    int32_t two[3] = { 7, 7, 7 };
    if (vp9hip_bicubic_weights(0, 4, 0, NULL, NULL, 0, NULL, NULL) != VP9HIP_EINVAL ||
        vp9hip_bicubic_weights(4, 16385, 0, NULL, NULL, 0, NULL, NULL) != VP9HIP_EINVAL ||
        vp9hip_bicubic_weights(16385, 4, 0, NULL, NULL, 0, NULL, NULL) != VP9HIP_EINVAL ||
        vp9hip_bicubic_weights(8, 4, 4, NULL, NULL, 0, NULL, NULL) != VP9HIP_EINVAL ||
        vp9hip_bicubic_weights(8, 4, -1, NULL, NULL, 0, NULL, NULL) != VP9HIP_EINVAL ||
        vp9hip_bicubic_weights(8, 4, 0, NULL, two, -1, NULL, NULL) != VP9HIP_EINVAL ||
        vp9hip_bicubic_weights(16, 8, 3, NULL, two, 2, NULL, NULL) != 8 || two[2] != 7 || two[0] == 7) {
        printf("argument checks\n");
        return 1;
    }
    printf("bicubic_weights_check OK: %ld weights\n", checked);
    return 0;
}
