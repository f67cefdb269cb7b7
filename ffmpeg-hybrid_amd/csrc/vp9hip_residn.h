/*
 * The 8-, 16- and 32-point inverse transforms of the residual kernels (k_resid's tx codes 1-3),
 * shared by the device kernels (vp9hip_kernels.hip: resid_wave) and the host entry
 * vp9hip_residn_host (the CPU check against the oracle, tests/test_resid_wave_host.py). One
 * restatement of the reference, two executors: every function is __host__ __device__.
 *
 *   idct8, iadst8      vp9dsp_template.c:1236-1314
 *   idct16, iadst16    vp9dsp_template.c:1318-1507
 *   idct32             vp9dsp_template.c:1511-1715
 *   tx1n               one 1-D pass of compile-time length
 * The arithmetic policies M32 / M64 and the 4-point transforms: vp9hip_resid4.h.
 * Internal to libvp9hip.
 */
#ifndef VP9HIP_RESIDN_H
#define VP9HIP_RESIDN_H
#include "vp9hip_resid4.h"

#define R(x) M::r14(x)
#define C(k) ((T) (k))

// vp9dsp_template.c:1236-1270
template <class M> R4_HD void idct8(typename M::T *io)
{
    typedef typename M::T T;
    T t0a = R((io[0] + io[4]) * C(11585)), t1a = R((io[0] - io[4]) * C(11585));
    T t2a = R(io[2] * C(6270) - io[6] * C(15137)), t3a = R(io[2] * C(15137) + io[6] * C(6270));
    T t4a = R(io[1] * C(3196) - io[7] * C(16069)), t5a = R(io[5] * C(13623) - io[3] * C(9102));
    T t6a = R(io[5] * C(9102) + io[3] * C(13623)), t7a = R(io[1] * C(16069) + io[7] * C(3196));
    T t0 = t0a + t3a, t1 = t1a + t2a, t2 = t1a - t2a, t3 = t0a - t3a;
    T t4 = t4a + t5a, t7 = t7a + t6a;
    t5a = t4a - t5a; t6a = t7a - t6a;
    T t5 = R((t6a - t5a) * C(11585)), t6 = R((t6a + t5a) * C(11585));
    io[0] = t0 + t7; io[1] = t1 + t6; io[2] = t2 + t5; io[3] = t3 + t4;
    io[4] = t3 - t4; io[5] = t2 - t5; io[6] = t1 - t6; io[7] = t0 - t7;
}
// vp9dsp_template.c:1272-1314
template <class M> R4_HD void iadst8(typename M::T *io)
{
    typedef typename M::T T;
    T t0a = C(16305) * io[7] + C(1606) * io[0], t1a = C(1606) * io[7] - C(16305) * io[0];
    T t2a = C(14449) * io[5] + C(7723) * io[2], t3a = C(7723) * io[5] - C(14449) * io[2];
    T t4a = C(10394) * io[3] + C(12665) * io[4], t5a = C(12665) * io[3] - C(10394) * io[4];
    T t6a = C(4756) * io[1] + C(15679) * io[6], t7a = C(15679) * io[1] - C(4756) * io[6];
    T t0 = R(t0a + t4a), t1 = R(t1a + t5a), t2 = R(t2a + t6a), t3 = R(t3a + t7a);
    T t4 = R(t0a - t4a), t5 = R(t1a - t5a), t6 = R(t2a - t6a), t7 = R(t3a - t7a);
    t4a = C(15137) * t4 + C(6270) * t5;
    t5a = C(6270) * t4 - C(15137) * t5;
    t6a = C(15137) * t7 - C(6270) * t6;
    t7a = C(6270) * t7 + C(15137) * t6;
    io[0] = t0 + t2;
    io[7] = C(0) - (t1 + t3);
    t2 = t0 - t2;
    t3 = t1 - t3;
    io[1] = C(0) - R(t4a + t6a);
    io[6] = R(t5a + t7a);
    t6 = R(t4a - t6a);
    t7 = R(t5a - t7a);
    io[3] = C(0) - R((t2 + t3) * C(11585));
    io[4] = R((t2 - t3) * C(11585));
    io[2] = R((t6 + t7) * C(11585));
    io[5] = C(0) - R((t6 - t7) * C(11585));
}
// vp9dsp_template.c:1318-1404
template <class M> R4_HD void idct16(typename M::T *io)
{
    typedef typename M::T T;
    T t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11, t12, t13, t14, t15;
    T t0a, t1a, t2a, t3a, t4a, t5a, t6a, t7a, t8a, t9a, t10a, t11a, t12a, t13a, t14a, t15a;
    t0a = R((io[0] + io[8]) * C(11585));
    t1a = R((io[0] - io[8]) * C(11585));
    t2a = R(io[4] * C(6270) - io[12] * C(15137));
    t3a = R(io[4] * C(15137) + io[12] * C(6270));
    t4a = R(io[2] * C(3196) - io[14] * C(16069));
    t7a = R(io[2] * C(16069) + io[14] * C(3196));
    t5a = R(io[10] * C(13623) - io[6] * C(9102));
    t6a = R(io[10] * C(9102) + io[6] * C(13623));
    t8a = R(io[1] * C(1606) - io[15] * C(16305));
    t15a = R(io[1] * C(16305) + io[15] * C(1606));
    t9a = R(io[9] * C(12665) - io[7] * C(10394));
    t14a = R(io[9] * C(10394) + io[7] * C(12665));
    t10a = R(io[5] * C(7723) - io[11] * C(14449));
    t13a = R(io[5] * C(14449) + io[11] * C(7723));
    t11a = R(io[13] * C(15679) - io[3] * C(4756));
    t12a = R(io[13] * C(4756) + io[3] * C(15679));
    t0 = t0a + t3a; t1 = t1a + t2a; t2 = t1a - t2a; t3 = t0a - t3a;
    t4 = t4a + t5a; t5 = t4a - t5a; t6 = t7a - t6a; t7 = t7a + t6a;
    t8 = t8a + t9a; t9 = t8a - t9a; t10 = t11a - t10a; t11 = t11a + t10a;
    t12 = t12a + t13a; t13 = t12a - t13a; t14 = t15a - t14a; t15 = t15a + t14a;
    t5a = R((t6 - t5) * C(11585));
    t6a = R((t6 + t5) * C(11585));
    t9a = R(t14 * C(6270) - t9 * C(15137));
    t14a = R(t14 * C(15137) + t9 * C(6270));
    t10a = R(C(0) - (t13 * C(15137) + t10 * C(6270)));
    t13a = R(t13 * C(6270) - t10 * C(15137));
    t0a = t0 + t7; t1a = t1 + t6a; t2a = t2 + t5a; t3a = t3 + t4;
    t4 = t3 - t4; t5 = t2 - t5a; t6 = t1 - t6a; t7 = t0 - t7;
    t8a = t8 + t11; t9 = t9a + t10a; t10 = t9a - t10a; t11a = t8 - t11;
    t12a = t15 - t12; t13 = t14a - t13a; t14 = t14a + t13a; t15a = t15 + t12;
    t10a = R((t13 - t10) * C(11585));
    t13a = R((t13 + t10) * C(11585));
    t11 = R((t12a - t11a) * C(11585));
    t12 = R((t12a + t11a) * C(11585));
    io[0] = t0a + t15a; io[1] = t1a + t14; io[2] = t2a + t13a; io[3] = t3a + t12;
    io[4] = t4 + t11; io[5] = t5 + t10a; io[6] = t6 + t9; io[7] = t7 + t8a;
    io[8] = t7 - t8a; io[9] = t6 - t9; io[10] = t5 - t10a; io[11] = t4 - t11;
    io[12] = t3a - t12; io[13] = t2a - t13a; io[14] = t1a - t14; io[15] = t0a - t15a;
}
// vp9dsp_template.c:1406-1507
template <class M> R4_HD void iadst16(typename M::T *io)
{
    typedef typename M::T T;
    T t0, t1, t2, t3, t4, t5, t6, t7, t8, t9, t10, t11, t12, t13, t14, t15;
    T t0a, t1a, t2a, t3a, t4a, t5a, t6a, t7a, t8a, t9a, t10a, t11a, t12a, t13a, t14a, t15a;
    t0 = io[15] * C(16364) + io[0] * C(804);
    t1 = io[15] * C(804) - io[0] * C(16364);
    t2 = io[13] * C(15893) + io[2] * C(3981);
    t3 = io[13] * C(3981) - io[2] * C(15893);
    t4 = io[11] * C(14811) + io[4] * C(7005);
    t5 = io[11] * C(7005) - io[4] * C(14811);
    t6 = io[9] * C(13160) + io[6] * C(9760);
    t7 = io[9] * C(9760) - io[6] * C(13160);
    t8 = io[7] * C(11003) + io[8] * C(12140);
    t9 = io[7] * C(12140) - io[8] * C(11003);
    t10 = io[5] * C(8423) + io[10] * C(14053);
    t11 = io[5] * C(14053) - io[10] * C(8423);
    t12 = io[3] * C(5520) + io[12] * C(15426);
    t13 = io[3] * C(15426) - io[12] * C(5520);
    t14 = io[1] * C(2404) + io[14] * C(16207);
    t15 = io[1] * C(16207) - io[14] * C(2404);
    t0a = R(t0 + t8); t1a = R(t1 + t9); t2a = R(t2 + t10); t3a = R(t3 + t11);
    t4a = R(t4 + t12); t5a = R(t5 + t13); t6a = R(t6 + t14); t7a = R(t7 + t15);
    t8a = R(t0 - t8); t9a = R(t1 - t9); t10a = R(t2 - t10); t11a = R(t3 - t11);
    t12a = R(t4 - t12); t13a = R(t5 - t13); t14a = R(t6 - t14); t15a = R(t7 - t15);
    t8 = t8a * C(16069) + t9a * C(3196);
    t9 = t8a * C(3196) - t9a * C(16069);
    t10 = t10a * C(9102) + t11a * C(13623);
    t11 = t10a * C(13623) - t11a * C(9102);
    t12 = t13a * C(16069) - t12a * C(3196);
    t13 = t13a * C(3196) + t12a * C(16069);
    t14 = t15a * C(9102) - t14a * C(13623);
    t15 = t15a * C(13623) + t14a * C(9102);
    t0 = t0a + t4a; t1 = t1a + t5a; t2 = t2a + t6a; t3 = t3a + t7a;
    t4 = t0a - t4a; t5 = t1a - t5a; t6 = t2a - t6a; t7 = t3a - t7a;
    t8a = R(t8 + t12); t9a = R(t9 + t13); t10a = R(t10 + t14); t11a = R(t11 + t15);
    t12a = R(t8 - t12); t13a = R(t9 - t13); t14a = R(t10 - t14); t15a = R(t11 - t15);
    t4a = t4 * C(15137) + t5 * C(6270);
    t5a = t4 * C(6270) - t5 * C(15137);
    t6a = t7 * C(15137) - t6 * C(6270);
    t7a = t7 * C(6270) + t6 * C(15137);
    t12 = t12a * C(15137) + t13a * C(6270);
    t13 = t12a * C(6270) - t13a * C(15137);
    t14 = t15a * C(15137) - t14a * C(6270);
    t15 = t15a * C(6270) + t14a * C(15137);
    io[0] = t0 + t2;
    io[15] = C(0) - (t1 + t3);
    t2a = t0 - t2;
    t3a = t1 - t3;
    io[3] = C(0) - R(t4a + t6a);
    io[12] = R(t5a + t7a);
    t6 = R(t4a - t6a);
    t7 = R(t5a - t7a);
    io[1] = C(0) - (t8a + t10a);
    io[14] = t9a + t11a;
    t10 = t8a - t10a;
    t11 = t9a - t11a;
    io[2] = R(t12 + t14);
    io[13] = C(0) - R(t13 + t15);
    t14a = R(t12 - t14);
    t15a = R(t13 - t15);
    io[7] = R((C(0) - (t2a + t3a)) * C(11585));
    io[8] = R((t2a - t3a) * C(11585));
    io[4] = R((t7 + t6) * C(11585));
    io[11] = R((t7 - t6) * C(11585));
    io[6] = R((t11 + t10) * C(11585));
    io[9] = R((t11 - t10) * C(11585));
    io[5] = R((C(0) - (t14a + t15a)) * C(11585));
    io[10] = R((t14a - t15a) * C(11585));
}
// vp9dsp_template.c:1511-1715
template <class M> R4_HD void idct32(typename M::T *io)
{
    typedef typename M::T T;
    T t0a = R((io[0] + io[16]) * C(11585));
    T t1a = R((io[0] - io[16]) * C(11585));
    T t2a = R(io[8] * C(6270) - io[24] * C(15137));
    T t3a = R(io[8] * C(15137) + io[24] * C(6270));
    T t4a = R(io[4] * C(3196) - io[28] * C(16069));
    T t7a = R(io[4] * C(16069) + io[28] * C(3196));
    T t5a = R(io[20] * C(13623) - io[12] * C(9102));
    T t6a = R(io[20] * C(9102) + io[12] * C(13623));
    T t8a = R(io[2] * C(1606) - io[30] * C(16305));
    T t15a = R(io[2] * C(16305) + io[30] * C(1606));
    T t9a = R(io[18] * C(12665) - io[14] * C(10394));
    T t14a = R(io[18] * C(10394) + io[14] * C(12665));
    T t10a = R(io[10] * C(7723) - io[22] * C(14449));
    T t13a = R(io[10] * C(14449) + io[22] * C(7723));
    T t11a = R(io[26] * C(15679) - io[6] * C(4756));
    T t12a = R(io[26] * C(4756) + io[6] * C(15679));
    T t16a = R(io[1] * C(804) - io[31] * C(16364));
    T t31a = R(io[1] * C(16364) + io[31] * C(804));
    T t17a = R(io[17] * C(12140) - io[15] * C(11003));
    T t30a = R(io[17] * C(11003) + io[15] * C(12140));
    T t18a = R(io[9] * C(7005) - io[23] * C(14811));
    T t29a = R(io[9] * C(14811) + io[23] * C(7005));
    T t19a = R(io[25] * C(15426) - io[7] * C(5520));
    T t28a = R(io[25] * C(5520) + io[7] * C(15426));
    T t20a = R(io[5] * C(3981) - io[27] * C(15893));
    T t27a = R(io[5] * C(15893) + io[27] * C(3981));
    T t21a = R(io[21] * C(14053) - io[11] * C(8423));
    T t26a = R(io[21] * C(8423) + io[11] * C(14053));
    T t22a = R(io[13] * C(9760) - io[19] * C(13160));
    T t25a = R(io[13] * C(13160) + io[19] * C(9760));
    T t23a = R(io[29] * C(16207) - io[3] * C(2404));
    T t24a = R(io[29] * C(2404) + io[3] * C(16207));

    T t0 = t0a + t3a, t1 = t1a + t2a, t2 = t1a - t2a, t3 = t0a - t3a;
    T t4 = t4a + t5a, t5 = t4a - t5a, t6 = t7a - t6a, t7 = t7a + t6a;
    T t8 = t8a + t9a, t9 = t8a - t9a, t10 = t11a - t10a, t11 = t11a + t10a;
    T t12 = t12a + t13a, t13 = t12a - t13a, t14 = t15a - t14a, t15 = t15a + t14a;
    T t16 = t16a + t17a, t17 = t16a - t17a, t18 = t19a - t18a, t19 = t19a + t18a;
    T t20 = t20a + t21a, t21 = t20a - t21a, t22 = t23a - t22a, t23 = t23a + t22a;
    T t24 = t24a + t25a, t25 = t24a - t25a, t26 = t27a - t26a, t27 = t27a + t26a;
    T t28 = t28a + t29a, t29 = t28a - t29a, t30 = t31a - t30a, t31 = t31a + t30a;

    t5a = R((t6 - t5) * C(11585));
    t6a = R((t6 + t5) * C(11585));
    t9a = R(t14 * C(6270) - t9 * C(15137));
    t14a = R(t14 * C(15137) + t9 * C(6270));
    t10a = R(C(0) - (t13 * C(15137) + t10 * C(6270)));
    t13a = R(t13 * C(6270) - t10 * C(15137));
    t17a = R(t30 * C(3196) - t17 * C(16069));
    t30a = R(t30 * C(16069) + t17 * C(3196));
    t18a = R(C(0) - (t29 * C(16069) + t18 * C(3196)));
    t29a = R(t29 * C(3196) - t18 * C(16069));
    t21a = R(t26 * C(13623) - t21 * C(9102));
    t26a = R(t26 * C(9102) + t21 * C(13623));
    t22a = R(C(0) - (t25 * C(9102) + t22 * C(13623)));
    t25a = R(t25 * C(13623) - t22 * C(9102));

    t0a = t0 + t7; t1a = t1 + t6a; t2a = t2 + t5a; t3a = t3 + t4;
    t4a = t3 - t4; t5 = t2 - t5a; t6 = t1 - t6a; t7a = t0 - t7;
    t8a = t8 + t11; t9 = t9a + t10a; t10 = t9a - t10a; t11a = t8 - t11;
    t12a = t15 - t12; t13 = t14a - t13a; t14 = t14a + t13a; t15a = t15 + t12;
    t16a = t16 + t19; t17 = t17a + t18a; t18 = t17a - t18a; t19a = t16 - t19;
    t20a = t23 - t20; t21 = t22a - t21a; t22 = t22a + t21a; t23a = t23 + t20;
    t24a = t24 + t27; t25 = t25a + t26a; t26 = t25a - t26a; t27a = t24 - t27;
    t28a = t31 - t28; t29 = t30a - t29a; t30 = t30a + t29a; t31a = t31 + t28;

    t10a = R((t13 - t10) * C(11585));
    t13a = R((t13 + t10) * C(11585));
    t11 = R((t12a - t11a) * C(11585));
    t12 = R((t12a + t11a) * C(11585));
    t18a = R(t29 * C(6270) - t18 * C(15137));
    t29a = R(t29 * C(15137) + t18 * C(6270));
    t19 = R(t28a * C(6270) - t19a * C(15137));
    t28 = R(t28a * C(15137) + t19a * C(6270));
    t20 = R(C(0) - (t27a * C(15137) + t20a * C(6270)));
    t27 = R(t27a * C(6270) - t20a * C(15137));
    t21a = R(C(0) - (t26 * C(15137) + t21 * C(6270)));
    t26a = R(t26 * C(6270) - t21 * C(15137));

    t0 = t0a + t15a; t1 = t1a + t14; t2 = t2a + t13a; t3 = t3a + t12;
    t4 = t4a + t11; t5a = t5 + t10a; t6a = t6 + t9; t7 = t7a + t8a;
    t8 = t7a - t8a; t9a = t6 - t9; t10 = t5 - t10a; t11a = t4a - t11;
    t12a = t3a - t12; t13 = t2a - t13a; t14a = t1a - t14; t15 = t0a - t15a;
    t16 = t16a + t23a; t17a = t17 + t22; t18 = t18a + t21a; t19a = t19 + t20;
    t20a = t19 - t20; t21 = t18a - t21a; t22a = t17 - t22; t23 = t16a - t23a;
    t24 = t31a - t24a; t25a = t30 - t25; t26 = t29a - t26a; t27a = t28 - t27;
    t28a = t28 + t27; t29 = t29a + t26a; t30a = t30 + t25; t31 = t31a + t24a;

    t20 = R((t27a - t20a) * C(11585));
    t27 = R((t27a + t20a) * C(11585));
    t21a = R((t26 - t21) * C(11585));
    t26a = R((t26 + t21) * C(11585));
    t22 = R((t25a - t22a) * C(11585));
    t25 = R((t25a + t22a) * C(11585));
    t23a = R((t24 - t23) * C(11585));
    t24a = R((t24 + t23) * C(11585));

    io[0] = t0 + t31; io[1] = t1 + t30a; io[2] = t2 + t29; io[3] = t3 + t28a;
    io[4] = t4 + t27; io[5] = t5a + t26a; io[6] = t6a + t25; io[7] = t7 + t24a;
    io[8] = t8 + t23a; io[9] = t9a + t22; io[10] = t10 + t21a; io[11] = t11a + t20;
    io[12] = t12a + t19a; io[13] = t13 + t18; io[14] = t14a + t17a; io[15] = t15 + t16;
    io[16] = t15 - t16; io[17] = t14a - t17a; io[18] = t13 - t18; io[19] = t12a - t19a;
    io[20] = t11a - t20; io[21] = t10 - t21a; io[22] = t9a - t22; io[23] = t8 - t23a;
    io[24] = t7 - t24a; io[25] = t6a - t25; io[26] = t5a - t26a; io[27] = t4 - t27;
    io[28] = t3 - t28a; io[29] = t2 - t29; io[30] = t1 - t30a; io[31] = t0 - t31;
}
#undef R
#undef C

// One 1-D inverse transform of compile-time length N (adst: 0 dct, 1 adst).
template <int N, class M> R4_HD void tx1n(typename M::T *v, int adst)
{
    if (N == 4) { if (adst) iadst4<M>(v); else idct4<M>(v); }
    else if (N == 8) { if (adst) iadst8<M>(v); else idct8<M>(v); }
    else if (N == 16) { if (adst) iadst16<M>(v); else idct16<M>(v); }
    else idct32<M>(v);
}

/* LDS row stride (coefficients) of an N x N block: padded so that the transposed store
 * (lane li writes row li) spreads over the banks: an odd number of dwords per row */
template <int N, typename COEF> struct RStride { static constexpr int S = N + (sizeof(COEF) == 2 ? 2 : 1); };

/* The coefficient block of resid_wave in LDS: N rows of S = RStride coefficients of ESZ bytes.
 * Byte offset in that image of the raster position pos = row * N + col that a scan table of
 * vp9_tables.h gives: what the kernels' gather tables hold, and what the host restatement
 * scatters by. */
template <int N, int S, int ESZ> R4_HD constexpr int rn_lds_off(int pos) { return ((pos / N) * S + pos % N) * ESZ; }

/* The gather of resid_wave: per round of 8 * N scan-order coefficients, lane li of a block takes
 * the eight at kb = k0 + 8 * li by wide loads, whatever eob is, as long as kb < eob. The loads
 * reach at most this many bytes from coefficient kb (int16: five dwords from the dword at or
 * below it; int32: two 16-byte loads), so past the last live coefficient of the arena they stay
 * inside its VP9HIP_COEF_PAD spare bytes. */
#define RN_READ_SPAN16 20
#define RN_READ_SPAN32 32
#endif
