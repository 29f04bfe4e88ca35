// The real harmonics of degree 4 and 6 two libraries share: libmw_boo.so (include/mw_boo.h) uses all 22 components,
// libmw_nuc.so (include/mw_nuc.h) the 13 of l = 6 (components 9 .. 21; the nine of l = 4 are dead code there).  Included after
// `#pragma clang fp contract(off)`: every product and sum below is spelled out, and both translation units get the same bits.
// Like mw_lib_cells.h it exports nothing; each library compiles its own copy.
#pragma once

namespace mwharm {

constexpr int kNY = 22;                           // 9 components of l = 4, then 13 of l = 6
constexpr int kY6 = 9;                            // the first component of l = 6
constexpr int kN6 = 13;

// c_lm = sqrt((2 - delta_m0) (l - m)! / (l + m)!)
constexpr double k41 = 0.31622776601683794, k42 = 0.07453559924999299, k43 = 0.019920476822239894, k44 = 0.0070429521227376385;
constexpr double k61 = 0.21821789023599236, k62 = 0.03450327796711771, k63 = 0.005750546327852952, k64 = 0.00104990131391452,
                 k65 = 0.00022383971222927231, k66 = 6.461695905544936e-05;

// The 22 components of the unit vector (x, y, z): c_lm P_l^(m)(z) Re / Im (x + i y)^m, order (l = 4: m = 0, 1c, 1s, ... 4c, 4s; l = 6
// likewise).  sum_m Y_lm(u) Y_lm(v) = P_l(u . v).
__device__ __forceinline__ void harmonics(double x, double y, double z, double (&Y)[kNY])
{
    const double z2 = z * z;
    const double c2 = __builtin_fma(x, x, -(y * y)), s2 = 2.0 * (x * y);
    const double c3 = __builtin_fma(c2, x, -(s2 * y)), s3 = __builtin_fma(c2, y, s2 * x);
    const double c4 = __builtin_fma(c3, x, -(s3 * y)), s4 = __builtin_fma(c3, y, s3 * x);
    const double c5 = __builtin_fma(c4, x, -(s4 * y)), s5 = __builtin_fma(c4, y, s4 * x);
    const double c6 = __builtin_fma(c5, x, -(s5 * y)), s6 = __builtin_fma(c5, y, s5 * x);
    const double p41 = z * __builtin_fma(17.5 * k41, z2, -7.5 * k41);
    const double p42 = __builtin_fma(52.5 * k42, z2, -7.5 * k42);
    const double p43 = (105.0 * k43) * z;
    Y[0] = __builtin_fma(__builtin_fma(4.375, z2, -3.75), z2, 0.375);
    Y[1] = p41 * x;  Y[2] = p41 * y;
    Y[3] = p42 * c2; Y[4] = p42 * s2;
    Y[5] = p43 * c3; Y[6] = p43 * s3;
    Y[7] = (105.0 * k44) * c4; Y[8] = (105.0 * k44) * s4;
    const double p61 = z * __builtin_fma(__builtin_fma(86.625 * k61, z2, -78.75 * k61), z2, 13.125 * k61);
    const double p62 = __builtin_fma(__builtin_fma(433.125 * k62, z2, -236.25 * k62), z2, 13.125 * k62);
    const double p63 = z * __builtin_fma(1732.5 * k63, z2, -472.5 * k63);
    const double p64 = __builtin_fma(5197.5 * k64, z2, -472.5 * k64);
    const double p65 = (10395.0 * k65) * z;
    Y[9] = __builtin_fma(__builtin_fma(__builtin_fma(14.4375, z2, -19.6875), z2, 6.5625), z2, -0.3125);
    Y[10] = p61 * x;  Y[11] = p61 * y;
    Y[12] = p62 * c2; Y[13] = p62 * s2;
    Y[14] = p63 * c3; Y[15] = p63 * s3;
    Y[16] = p64 * c4; Y[17] = p64 * s4;
    Y[18] = p65 * c5; Y[19] = p65 * s5;
    Y[20] = (10395.0 * k66) * c6; Y[21] = (10395.0 * k66) * s6;
}

__device__ __forceinline__ void unit_harmonics(double r2, double dx, double dy, double dz, double (&Y)[kNY])
{
    const double rinv = 1.0 / __builtin_sqrt(r2);
    harmonics(dx * rinv, dy * rinv, dz * rinv, Y);
}

// sqrt of the sum of v[k]^2, k = first .. first + count - 1, added in that order
__device__ __forceinline__ double norm_of(const double* v, int first, int count)
{
    double s = 0.0;
    for (int k = first; k < first + count; ++k) s = __builtin_fma(v[k], v[k], s);
    return __builtin_sqrt(s);
}

}  // namespace mwharm
