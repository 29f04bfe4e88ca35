// libmw_hess.so -- the second derivatives of include/mw_hess.h: products of the Hessian of the full-box mW energy with given
// vectors and the dense Gamma-point Hessian, every box of a call on its own.  One geometry for every nwater: the counting sort
// of mw_lib_cells.h, k_hess_moments (one lane per molecule in sorted order walks the 27 cells: the ten moments and the molecule's
// energy), k_hess_forces and k_hess_ef (the energy and the largest force component of the box, where the caller asks for them).
// Products: k_hess_gather (a group of vectors into sorted order), k_hess_dmoments (the perturbed moments dM_i = sum_k J_k (v_jk - v_i))
// and k_hess_apply (a second walk over the moments and perturbed moments of the molecule and of every entry: (H v)_i, written by
// index).  Dense: k_hess_jsum (G_i = sum_k J_k, column by column), k_hess_clear and k_hess_rows (one wavefront per row molecule owns its
// 3 x 3 nwater strip: its first lane adds the blocks of the centres that touch the molecule in the order of the walk).  The
// arithmetic is spelled out in fma / mul / add with contraction off, every sum has a fixed order and there is no
// floating-point atomic (mw_hess.h).  The moments, the first derivatives and the reductions are those of mw_lib_forces.h,
// shared with the inherent-structure and molecular-dynamics libraries; the second derivatives are here.
#include "../../include/mw_hess.h"

#include "mw_common.hip.h"

#include <climits>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

#include "mw_lib_host.h"                       // after the pragma: its host arithmetic is uncontracted too
#include "mw_lib_cells.h"
#include "mw_lib_forces.h"                     // Sums, entry_force, CellRegs and the reductions

namespace mwhess {

using namespace mwcells;
using namespace mwforces;

constexpr int kPart = 2;                          // a workgroup's partial sums: E and the largest |F| component
constexpr int kLds = 64 * (4 + 9 * 8);            // the largest of the kernels: the column table of k_hess_rows (the counting sort's scan has 1024 bytes)
constexpr int kDm = 10;                           // a perturbed-moment record: dS0, dS1 (3), dS2 (xx, yy, zz, xy, xz, yz)
constexpr double kTwoCos0 = 2.0 * mw::kCos0;
constexpr size_t kClearBlocks = 16384;          // k_hess_clear strides beyond this many workgroups

// ---- the second derivatives ----------------------------------------------------------------------------------------------
// A ten-vector against which f(d) = g (1, u, u (x) u) is contracted: y0, y1 and the symmetric matrix Y2 (all six entries).
struct Vec10 {
    double y0, y1x, y1y, y1z, xx, yy, zz, xy, xz, yz;
};

// W M of a moment record of mw_lib_forces.h (S2 without zz: the u_k are unit vectors): (cos0^2 S0, -2 cos0 S1, S2)
__device__ __forceinline__ Vec10 weighted_moments(const double (&M)[kMom])
{
    Vec10 y;
    y.y0 = kCos0Sq * M[0];
    y.y1x = -kTwoCos0 * M[1]; y.y1y = -kTwoCos0 * M[2]; y.y1z = -kTwoCos0 * M[3];
    y.xx = M[4]; y.yy = M[5]; y.zz = (M[0] - M[4]) - M[5];
    y.xy = M[6]; y.xz = M[7]; y.yz = M[8];
    return y;
}

// W dM of a perturbed-moment record
__device__ __forceinline__ Vec10 weighted_record(const double* __restrict__ m)
{
    const double2* m2 = reinterpret_cast<const double2*>(m);
    const double2 a = m2[0], b = m2[1], c = m2[2], d = m2[3], e = m2[4];
    Vec10 y;
    y.y0 = kCos0Sq * a.x;
    y.y1x = -kTwoCos0 * a.y; y.y1y = -kTwoCos0 * b.x; y.y1z = -kTwoCos0 * b.y;
    y.xx = c.x; y.yy = c.y; y.zz = d.x; y.xy = d.y; y.xz = e.x; y.yz = e.y;
    return y;
}

// The sum of J w over the entries of a centre (or one J w from zero), in the layout of a perturbed-moment record.
struct DMom {
    double s0 = 0.0, s1x = 0.0, s1y = 0.0, s1z = 0.0, xx = 0.0, yy = 0.0, zz = 0.0, xy = 0.0, xz = 0.0, yz = 0.0;
    __device__ __forceinline__ Vec10 weighted() const
    {
        Vec10 y;
        y.y0 = kCos0Sq * s0;
        y.y1x = -kTwoCos0 * s1x; y.y1y = -kTwoCos0 * s1y; y.y1z = -kTwoCos0 * s1z;
        y.xx = xx; y.yy = yy; y.zz = zz; y.xy = xy; y.xz = xz; y.yz = yz;
        return y;
    }
    __device__ __forceinline__ void store(double* __restrict__ m) const
    {
        double2* w = reinterpret_cast<double2*>(m);
        w[0] = make_double2(s0, s1x); w[1] = make_double2(s1y, s1z); w[2] = make_double2(xx, yy);
        w[3] = make_double2(zz, xy);  w[4] = make_double2(xz, yz);
    }
};

// An entry at d, |d|^2 = r2 < (a sigma)^2, seen from its centre (SIGN = 1) or, as the entry -d of the neighbour's list, from the
// neighbour (SIGN = -1): u, 1 / r, g and its first two derivatives, and the first two derivatives of the radial part
//   psi(r) = 1/2 phi - 1/2 lambda eps (1 - cos0)^2 g^2.
// phi = c e1, c = A eps (B sigma^4 r^-4 - 1), e1 = exp(sigma w), g = exp(gamma sigma w), w = 1 / (r - a sigma) clamped as in pair_terms
// (past the clamp e1 = g = 0 and every derivative is exactly 0): e1' = -sigma w^2 e1, e1'' = e1 (sigma^2 w^4 + 2 sigma w^3), g alike.
struct Entry {
    double ux, uy, uz, rinv, g, dg, d2g, psi1, psi2;
};

template <int SIGN>
__device__ __forceinline__ Entry make_entry(double r2, double dx, double dy, double dz)
{
    Entry e;
    double e1;
    mw::pair_terms(r2, e.rinv, e1, e.g);
    const double w = mw::fast_rcp(__builtin_fmin(__builtin_fma(r2, e.rinv, -mw::kSigA), mw::kDenClamp));
    const double w2 = w * w, w3 = w2 * w, w4 = w2 * w2;
    const double ri2 = e.rinv * e.rinv, ri4 = ri2 * ri2;
    const double sr = SIGN * e.rinv;
    e.ux = dx * sr; e.uy = dy * sr; e.uz = dz * sr;
    e.dg = -mw::kGamSig * e.g * w2;
    e.d2g = e.g * __builtin_fma(mw::kGamSig * mw::kGamSig, w4, 2.0 * mw::kGamSig * w3);
    const double de1 = -mw::kSigma * e1 * w2;
    const double d2e1 = e1 * __builtin_fma(mw::kSigSq, w4, 2.0 * mw::kSigma * w3);
    const double c = __builtin_fma(ri4, kAepsBSig4, -mw::kAeps);
    const double dc = -4.0 * kAepsBSig4 * ri4 * e.rinv;
    const double d2c = 20.0 * kAepsBSig4 * ri4 * ri2;
    const double dphi = __builtin_fma(dc, e1, c * de1);
    const double d2phi = __builtin_fma(d2c, e1, __builtin_fma(2.0 * dc, de1, c * d2e1));
    constexpr double q = mw::kLamEps * kOneMinusCos0Sq;
    e.psi1 = __builtin_fma(0.5, dphi, -q * (e.g * e.dg));
    e.psi2 = __builtin_fma(0.5, d2phi, -q * __builtin_fma(e.dg, e.dg, e.g * e.d2g));
    return e;
}

// The same entry seen from the other end: d -> -d changes u alone (the bits of make_entry<-SIGN>).
__device__ __forceinline__ Entry flipped(const Entry& e)
{
    Entry f = e;
    f.ux = -e.ux; f.uy = -e.uy; f.uz = -e.uz;
    return f;
}

// a += J w: with s = u . w, p = w - s u and q = (g / r) p:  dS0 = g' s,  dS1 = g' s u + q,  dS2 = g' s u u^T + q u^T + u q^T
__device__ __forceinline__ void add_jw(const Entry& e, double wx, double wy, double wz, DMom& a)
{
    const double s = __builtin_fma(e.ux, wx, __builtin_fma(e.uy, wy, e.uz * wz));
    const double gr = e.g * e.rinv, t = e.dg * s;
    const double qx = gr * __builtin_fma(-s, e.ux, wx), qy = gr * __builtin_fma(-s, e.uy, wy), qz = gr * __builtin_fma(-s, e.uz, wz);
    const double tx = t * e.ux, ty = t * e.uy, tz = t * e.uz;
    a.s0 = a.s0 + t;
    a.s1x = a.s1x + (tx + qx); a.s1y = a.s1y + (ty + qy); a.s1z = a.s1z + (tz + qz);
    a.xx = a.xx + __builtin_fma(tx, e.ux, 2.0 * (qx * e.ux));
    a.yy = a.yy + __builtin_fma(ty, e.uy, 2.0 * (qy * e.uy));
    a.zz = a.zz + __builtin_fma(tz, e.uz, 2.0 * (qz * e.uz));
    a.xy = a.xy + __builtin_fma(tx, e.uy, __builtin_fma(qx, e.uy, e.ux * qy));
    a.xz = a.xz + __builtin_fma(tx, e.uz, __builtin_fma(qx, e.uz, e.ux * qz));
    a.yz = a.yz + __builtin_fma(ty, e.uz, __builtin_fma(qy, e.uz, e.uy * qz));
}

// What the contraction of f with y needs at u: Y2 u, A = y0 + y1 . u + u^T Y2 u, z = y1 + 2 Y2 u, u . z
struct Contraction {
    double A, zx, zy, zz, uz;
};
__device__ __forceinline__ Contraction contract(const Entry& e, const Vec10& y)
{
    const double ax = __builtin_fma(y.xx, e.ux, __builtin_fma(y.xy, e.uy, y.xz * e.uz));
    const double ay = __builtin_fma(y.xy, e.ux, __builtin_fma(y.yy, e.uy, y.yz * e.uz));
    const double az = __builtin_fma(y.xz, e.ux, __builtin_fma(y.yz, e.uy, y.zz * e.uz));
    Contraction c;
    const double uau = __builtin_fma(e.ux, ax, __builtin_fma(e.uy, ay, e.uz * az));
    const double uy1 = __builtin_fma(e.ux, y.y1x, __builtin_fma(e.uy, y.y1y, e.uz * y.y1z));
    c.A = y.y0 + (uy1 + uau);
    c.zx = __builtin_fma(2.0, ax, y.y1x); c.zy = __builtin_fma(2.0, ay, y.y1y); c.zz = __builtin_fma(2.0, az, y.y1z);
    c.uz = __builtin_fma(e.ux, c.zx, __builtin_fma(e.uy, c.zy, e.uz * c.zz));
    return c;
}

// J^T y = the gradient of h(d) = y . f(d):  g' A u + (g / r) (z - (u . z) u)
__device__ __forceinline__ void grad_h(const Entry& e, const Vec10& y, double& hx, double& hy, double& hz)
{
    const Contraction c = contract(e, y);
    const double p = e.dg * c.A, gr = e.g * e.rinv;
    hx = __builtin_fma(p, e.ux, gr * __builtin_fma(-c.uz, e.ux, c.zx));
    hy = __builtin_fma(p, e.uy, gr * __builtin_fma(-c.uz, e.uy, c.zy));
    hz = __builtin_fma(p, e.uz, gr * __builtin_fma(-c.uz, e.uz, c.zz));
}

// K w: the change along w of the gradient of psi(r) + lambda eps y . f(d), y = W M held fixed.  With s = u . w, du = (w - s u) / r,
// t = z - (u . z) u:  d(grad h) = g'' s A u + g' dA u + g' A du + d(g / r) t + (g / r) dt,  dA = z . du,  dz = 2 Y2 du,
// dt = dz - (du . z + u . dz) u - (u . z) du,  d(g / r) = (g' / r - g / r^2) s;  d(grad psi) = psi'' s u + psi' du.
__device__ __forceinline__ void apply_k(const Entry& e, const Vec10& y, double wx, double wy, double wz, double& kx, double& ky, double& kz)
{
    const Contraction c = contract(e, y);
    const double s = __builtin_fma(e.ux, wx, __builtin_fma(e.uy, wy, e.uz * wz));
    const double dux = e.rinv * __builtin_fma(-s, e.ux, wx), duy = e.rinv * __builtin_fma(-s, e.uy, wy), duz = e.rinv * __builtin_fma(-s, e.uz, wz);
    const double dzx = 2.0 * __builtin_fma(y.xx, dux, __builtin_fma(y.xy, duy, y.xz * duz));
    const double dzy = 2.0 * __builtin_fma(y.xy, dux, __builtin_fma(y.yy, duy, y.yz * duz));
    const double dzz = 2.0 * __builtin_fma(y.xz, dux, __builtin_fma(y.yz, duy, y.zz * duz));
    const double dA = __builtin_fma(c.zx, dux, __builtin_fma(c.zy, duy, c.zz * duz));
    const double udz = __builtin_fma(e.ux, dzx, __builtin_fma(e.uy, dzy, e.uz * dzz));
    const double m = dA + udz;                                          // du . z + u . dz
    const double gr = e.g * e.rinv;
    const double dgr = (e.dg * e.rinv - gr * e.rinv) * s;
    const double cu = __builtin_fma(e.d2g * s, c.A, e.dg * dA);          // the coefficient of u
    const double cd = e.dg * c.A;                                       // the coefficient of du
    const double tx = __builtin_fma(-c.uz, e.ux, c.zx), ty = __builtin_fma(-c.uz, e.uy, c.zy), tz = __builtin_fma(-c.uz, e.uz, c.zz);
    const double dtx = __builtin_fma(-c.uz, dux, __builtin_fma(-m, e.ux, dzx));
    const double dty = __builtin_fma(-c.uz, duy, __builtin_fma(-m, e.uy, dzy));
    const double dtz = __builtin_fma(-c.uz, duz, __builtin_fma(-m, e.uz, dzz));
    const double hx = __builtin_fma(cu, e.ux, __builtin_fma(cd, dux, __builtin_fma(dgr, tx, gr * dtx)));
    const double hy = __builtin_fma(cu, e.uy, __builtin_fma(cd, duy, __builtin_fma(dgr, ty, gr * dty)));
    const double hz = __builtin_fma(cu, e.uz, __builtin_fma(cd, duz, __builtin_fma(dgr, tz, gr * dtz)));
    const double ps = e.psi2 * s;
    kx = __builtin_fma(mw::kLamEps, hx, __builtin_fma(ps, e.ux, e.psi1 * dux));
    ky = __builtin_fma(mw::kLamEps, hy, __builtin_fma(ps, e.uy, e.psi1 * duy));
    kz = __builtin_fma(mw::kLamEps, hz, __builtin_fma(ps, e.uz, e.psi1 * duz));
}

// ---- the passes both entries share -----------------------------------------------------------------------------------------
// Per box in scratch after the sort's pieces (mw_lib_cells.h): mom [n][kMom] and en [n] in cell order, part [workgroups][kPart].

// The moment pass, one lane per molecule in sorted order.
__global__ __launch_bounds__(kThreads) void k_hess_moments(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                           const int* __restrict__ start, const double* __restrict__ ss, double* __restrict__ mom,
                                                           double* __restrict__ en)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    Sums a;
    const CellRegs hc(par + 18 * (size_t)b);
    walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
               [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                   if (q == p) return;                                 // (an own image: beyond the cutoff in the supported range)
                   a.add(r2, dx, dy, dz);
               });
    double M[kMom];
    a.record(M);
    double2* w = reinterpret_cast<double2*>(mom + kMom * (o + p));
#pragma unroll
    for (int c = 0; c < kMom / 2; ++c) w[c] = make_double2(M[2 * c], M[2 * c + 1]);
    en[o + p] = a.energy();
}

// The force pass behind ef, one lane per molecule in sorted order: the workgroup's sum of the energies and its largest |F|
// component.
__global__ __launch_bounds__(kThreads) void k_hess_forces(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                          const int* __restrict__ start, const double* __restrict__ ss, const double* __restrict__ mom,
                                                          const double* __restrict__ en, double* __restrict__ part)
{
    __shared__ double red[kThreads / 64][kPart];
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    const size_t o = (size_t)b * n;
    double val[kPart] = {0.0, 0.0};
    if (p < n) {
        const double* S = ss + 3 * o;
        const double* Mb = mom + kMom * o;
        const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
        double Mi[kMom];
        mw::load_moments(Mb + kMom * (size_t)p, Mi);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        const CellRegs hc(par + 18 * (size_t)b);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
                   [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                       if (q == p) return;
                       double Mj[kMom];
                       mw::load_moments(Mb + kMom * (size_t)q, Mj);
                       entry_force(Mi, Mj, r2, dx, dy, dz, fx, fy, fz);
                   });
        val[0] = en[o + p];
        const double ax = __builtin_fabs(fx), ay = __builtin_fabs(fy), az = __builtin_fabs(fz);
        val[1] = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
    }
    const double r = block_reduce<1, 1>(val, red);
    if (threadIdx.x < kPart) part[((size_t)b * gridDim.x + blockIdx.x) * kPart + threadIdx.x] = r;
}

// One wavefront per box: lane k < kPart takes column k of the box's partials in workgroup order.
__global__ __launch_bounds__(64) void k_hess_ef(int nwg, const double* __restrict__ part, double* __restrict__ ef)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= kPart) return;
    const double* P = part + (size_t)b * nwg * kPart;
    double a = P[k];
    for (int w = 1; w < nwg; ++w) {
        const double t = P[(size_t)w * kPart + k];
        a = k == 0 ? a + t : (t > a ? t : a);
    }
    ef[kPart * (size_t)b + k] = a;
}

// ---- products -----------------------------------------------------------------------------------------------------------------
// A group of nvg vectors, blockIdx.z the vector: vs [box][nvg][n][3] in cell order and dmom [box][nvg][n][kDm] in scratch; vecs
// and out are reached through the strides (in doubles) from one box to the next.

__global__ __launch_bounds__(kThreads) void k_hess_gather(int n, const int* __restrict__ idx, const double* __restrict__ vecs, size_t box_stride,
                                                          double* __restrict__ vs)
{
    const int b = blockIdx.y, z = blockIdx.z, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* v = vecs + (size_t)b * box_stride + 3 * (size_t)n * z + 3 * (size_t)idx[(size_t)b * n + p];
    double* w = vs + 3 * (((size_t)b * gridDim.z + z) * n + p);
    w[0] = v[0]; w[1] = v[1]; w[2] = v[2];
}

// The perturbed moments, one lane per molecule in sorted order.
__global__ __launch_bounds__(kThreads) void k_hess_dmoments(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                            const int* __restrict__ start, const double* __restrict__ ss, const double* __restrict__ vs,
                                                            double* __restrict__ dmom)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* S = ss + 3 * (size_t)b * n;
    const size_t ov = ((size_t)b * gridDim.z + blockIdx.z) * n;
    const double* V = vs + 3 * ov;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    const double vx = V[3 * (size_t)p], vy = V[3 * (size_t)p + 1], vz = V[3 * (size_t)p + 2];
    DMom a;
    const CellRegs hc(par + 18 * (size_t)b);
    walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
               [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                   if (q == p) return;
                   const Entry e = make_entry<1>(r2, dx, dy, dz);
                   add_jw(e, V[3 * (size_t)q] - vx, V[3 * (size_t)q + 1] - vy, V[3 * (size_t)q + 2] - vz, a);
               });
    a.store(dmom + kDm * (ov + p));
}

// (H v)_i, one lane per molecule in sorted order.  The entry k of i at d with w = v_j - v_i: the centre i gives
// a = lambda eps J(d)^T W dM_i + K(d; M_i) w, the centre j, whose entry -d points back, b = lambda eps J(-d)^T W dM_j - K(-d; M_j) w, and
// (H v)_i = sum_k (b - a).
__global__ __launch_bounds__(kThreads) void k_hess_apply(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                         const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ idx,
                                                         const double* __restrict__ mom, const double* __restrict__ vs, const double* __restrict__ dmom,
                                                         double* __restrict__ out, size_t box_stride)
{
    const int b = blockIdx.y, z = blockIdx.z, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const size_t o = (size_t)b * n, ov = ((size_t)b * gridDim.z + z) * n;
    const double* S = ss + 3 * o;
    const double* Mb = mom + kMom * o;
    const double* V = vs + 3 * ov;
    const double* Db = dmom + kDm * ov;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    const double vx = V[3 * (size_t)p], vy = V[3 * (size_t)p + 1], vz = V[3 * (size_t)p + 2];
    double Mi[kMom];
    mw::load_moments(Mb + kMom * (size_t)p, Mi);
    const Vec10 yi = weighted_moments(Mi), di = weighted_record(Db + kDm * (size_t)p);
    double hx = 0.0, hy = 0.0, hz = 0.0;
    const CellRegs hc(par + 18 * (size_t)b);
    walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
               [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                   if (q == p) return;
                   const double wx = V[3 * (size_t)q] - vx, wy = V[3 * (size_t)q + 1] - vy, wz = V[3 * (size_t)q + 2] - vz;
                   double gx, gy, gz, kx, ky, kz;
                   const Entry e = make_entry<1>(r2, dx, dy, dz);
                   grad_h(e, di, gx, gy, gz);
                   apply_k(e, yi, wx, wy, wz, kx, ky, kz);
                   const double ax = __builtin_fma(mw::kLamEps, gx, kx), ay = __builtin_fma(mw::kLamEps, gy, ky), az = __builtin_fma(mw::kLamEps, gz, kz);
                   double Mj[kMom];
                   mw::load_moments(Mb + kMom * (size_t)q, Mj);
                   const Vec10 yj = weighted_moments(Mj), dj = weighted_record(Db + kDm * (size_t)q);
                   const Entry f = flipped(e);
                   grad_h(f, dj, gx, gy, gz);
                   apply_k(f, yj, -wx, -wy, -wz, kx, ky, kz);
                   const double bx = __builtin_fma(mw::kLamEps, gx, kx), by = __builtin_fma(mw::kLamEps, gy, ky), bz = __builtin_fma(mw::kLamEps, gz, kz);
                   hx = hx + (bx - ax); hy = hy + (by - ay); hz = hz + (bz - az);
               });
    double* w = out + (size_t)b * box_stride + 3 * (size_t)n * z + 3 * (size_t)idx[o + p];
    w[0] = hx; w[1] = hy; w[2] = hz;
}

// ---- the dense matrix ---------------------------------------------------------------------------------------------------------
// gsum [n][3][kDm] in cell order: column c of G_i = sum_k J_k, the perturbed moments of the centre i for e_c on every entry.
__global__ __launch_bounds__(kThreads) void k_hess_jsum(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                        const int* __restrict__ start, const double* __restrict__ ss, double* __restrict__ gsum)
{
    const int b = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const double* S = ss + 3 * (size_t)b * n;
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    DMom gx, gy, gz;
    const CellRegs hc(par + 18 * (size_t)b);
    walk_cells(s0, s1, s2, mw::kRcSq, hc.c, grid + 4 * (size_t)b, start + (size_t)b * (cap + 1), S,
               [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
                   if (q == p) return;
                   const Entry e = make_entry<1>(r2, dx, dy, dz);
                   add_jw(e, 1.0, 0.0, 0.0, gx);
                   add_jw(e, 0.0, 1.0, 0.0, gy);
                   add_jw(e, 0.0, 0.0, 1.0, gz);
               });
    double* w = gsum + 3 * kDm * ((size_t)b * n + p);
    gx.store(w); gy.store(w + kDm); gz.store(w + 2 * kDm);
}

// The strip of a row molecule while its blocks are added: the first kSlots distinct columns live in a table in LDS (open
// addressing from j mod kSlots, a column's nine doubles beside its key), any further column in the cleared strip itself.  A
// column always takes the same path, so its sum runs in the order of the additions either way.
constexpr int kSlots = 64;
static_assert(kLds == kSlots * (4 + 9 * 8), "the plan reports the table of k_hess_rows");
struct Strip {
    int* keys;                                    // [kSlots], -1: free
    double* vals;                                 // [kSlots][9]
    double* row;
    size_t ld;
    // block (a, c) of column j += sgn m[a][c]
    __device__ __forceinline__ void add(int j, double sgn, const double (&m)[3][3]) const
    {
        int s = j & (kSlots - 1), tried = 0;
        while (tried < kSlots && keys[s] != j && keys[s] >= 0) { s = (s + 1) & (kSlots - 1); ++tried; }
        if (tried < kSlots) {
            keys[s] = j;
            double* v = vals + 9 * s;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[3 * a + c] = __builtin_fma(sgn, m[a][c], v[3 * a + c]);
            return;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double* r = row + a * ld + 3 * (size_t)j;                  // (one lane's own earlier stores are what it reads back)
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = __builtin_fma(sgn, m[a][c], r[c]);
        }
    }
};

// Clears `count` doubles from p on, 16 bytes per lane where p allows it.
__global__ __launch_bounds__(kThreads) void k_hess_clear(double* __restrict__ p, size_t count)
{
    const size_t head = ((size_t)p & 8) && count ? 1 : 0, pairs = (count - head) / 2;
    double2* q = reinterpret_cast<double2*>(p + head);
    const size_t step = (size_t)gridDim.x * kThreads;
    for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < pairs; t += step) q[t] = make_double2(0.0, 0.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) p[0] = 0.0;
        if (head + 2 * pairs < count) p[count - 1] = 0.0;
    }
}

// One wavefront per row molecule (sorted place p = blockIdx.x, molecule i = idx[p]): it owns the strip hess[3 i .. 3 i + 2][*],
// which k_hess_clear has cleared.  Its first lane adds (assemble_row), in the order of the walk:
//   the centre i, for its entry l:  R = sum_k B_kl, row a of which is lambda eps J_l^T W G_i[a] + K_l[a] (B_lk = B_kl^T):
//       -R to column j_l, +R to column i;
//   every centre c that has i among its entries (the entry k of c at -d, for the entry of i at d):  K_k to column i,
//       -(lambda eps J_k^T W G_c + K_k) to column c, and for every entry l of c  lambda eps J_k^T W J_l to column j_l;
// then lane t writes the column of slot t of the table into the strip.
__device__ __forceinline__ void assemble_row(int n, int cap, int b, int p, int i, const Strip& strip, const double* __restrict__ par,
                                             const int* __restrict__ grid, const int* __restrict__ start, const double* __restrict__ ss,
                                             const int* __restrict__ idx, const double* __restrict__ mom, const double* __restrict__ gsum)
{
    const size_t o = (size_t)b * n;
    const double* S = ss + 3 * o;
    const double* Mb = mom + kMom * o;
    const double* Gb = gsum + 3 * kDm * o;
    const int* ix = idx + o;
    const int* g = grid + 4 * (size_t)b;
    const int* st = start + (size_t)b * (cap + 1);
    const double s0 = S[3 * (size_t)p], s1 = S[3 * (size_t)p + 1], s2 = S[3 * (size_t)p + 2];
    const CellRegs hc(par + 18 * (size_t)b);
    {
        double Mi[kMom];
        mw::load_moments(Mb + kMom * (size_t)p, Mi);
        const Vec10 yi = weighted_moments(Mi);
        const Vec10 g0 = weighted_record(Gb + 3 * kDm * (size_t)p), g1 = weighted_record(Gb + 3 * kDm * (size_t)p + kDm),
                    g2 = weighted_record(Gb + 3 * kDm * (size_t)p + 2 * kDm);
        walk_cells(s0, s1, s2, mw::kRcSq, hc.c, g, st, S, [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
            if (q == p) return;
            const Entry e = make_entry<1>(r2, dx, dy, dz);
            double R[3][3], K[3][3];
            grad_h(e, g0, R[0][0], R[0][1], R[0][2]);
            grad_h(e, g1, R[1][0], R[1][1], R[1][2]);
            grad_h(e, g2, R[2][0], R[2][1], R[2][2]);
            apply_k(e, yi, 1.0, 0.0, 0.0, K[0][0], K[1][0], K[2][0]);
            apply_k(e, yi, 0.0, 1.0, 0.0, K[0][1], K[1][1], K[2][1]);
            apply_k(e, yi, 0.0, 0.0, 1.0, K[0][2], K[1][2], K[2][2]);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c) R[a][c] = __builtin_fma(mw::kLamEps, R[a][c], K[a][c]);
            strip.add(ix[q], -1.0, R);
            strip.add(i, 1.0, R);
        });
    }
    walk_cells(s0, s1, s2, mw::kRcSq, hc.c, g, st, S, [&](int q, int, int, int, double r2, double dx, double dy, double dz) {
        if (q == p) return;
        const Entry e = flipped(make_entry<1>(r2, dx, dy, dz));        // the entry of the centre q that points to i
        double K[3][3], C[3][3];
        {
            double Mc[kMom];
            mw::load_moments(Mb + kMom * (size_t)q, Mc);
            const Vec10 yc = weighted_moments(Mc);
            apply_k(e, yc, 1.0, 0.0, 0.0, K[0][0], K[1][0], K[2][0]);
            apply_k(e, yc, 0.0, 1.0, 0.0, K[0][1], K[1][1], K[2][1]);
            apply_k(e, yc, 0.0, 0.0, 1.0, K[0][2], K[1][2], K[2][2]);
        }
        strip.add(i, 1.0, K);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Vec10 gc = weighted_record(Gb + 3 * kDm * (size_t)q + kDm * c);
            double x, y, z;
            grad_h(e, gc, x, y, z);
            C[0][c] = __builtin_fma(mw::kLamEps, x, K[0][c]); C[1][c] = __builtin_fma(mw::kLamEps, y, K[1][c]); C[2][c] = __builtin_fma(mw::kLamEps, z, K[2][c]);
        }
        strip.add(ix[q], -1.0, C);
        const double t0 = S[3 * (size_t)q], t1 = S[3 * (size_t)q + 1], t2 = S[3 * (size_t)q + 2];
        walk_cells(t0, t1, t2, mw::kRcSq, hc.c, g, st, S, [&](int l, int, int, int, double q2, double ex, double ey, double ez) {
            if (l == q) return;
            const Entry f = make_entry<1>(q2, ex, ey, ez);
            double B[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                DMom jw;
                add_jw(f, c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, jw);
                double x, y, z;
                grad_h(e, jw.weighted(), x, y, z);
                B[0][c] = mw::kLamEps * x; B[1][c] = mw::kLamEps * y; B[2][c] = mw::kLamEps * z;
            }
            strip.add(ix[l], 1.0, B);
        });
    });
}

__global__ __launch_bounds__(64) void k_hess_rows(int n, int cap, const double* __restrict__ par, const int* __restrict__ grid,
                                                  const int* __restrict__ start, const double* __restrict__ ss, const int* __restrict__ idx,
                                                  const double* __restrict__ mom, const double* __restrict__ gsum, double* __restrict__ hess)
{
    __shared__ int keys[kSlots];
    __shared__ double vals[kSlots][9];
    const int b = blockIdx.y, p = blockIdx.x, t = threadIdx.x;
    const size_t ld = 3 * (size_t)n;
    const int i = idx[(size_t)b * n + p];
    double* row = hess + (size_t)b * ld * ld + 3 * (size_t)i * ld;
    keys[t] = -1;
#pragma unroll
    for (int k = 0; k < 9; ++k) vals[t][k] = 0.0;
    __syncthreads();
    if (t == 0) assemble_row(n, cap, b, p, i, Strip{keys, &vals[0][0], row, ld}, par, grid, start, ss, idx, mom, gsum);
    __syncthreads();
    const int j = keys[t];
    if (j < 0) return;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) row[a * ld + 3 * (size_t)j + c] = vals[t][3 * a + c];
}

}  // namespace mwhess

namespace {

using namespace mwhess;

struct State : Runtime<5> {
    Buf scratch, par, grid, pos, vecs, out, ef;
    int last[MW_HESS_PLAN_FIELDS] = {0};
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
} g;

// The scratch of one box: the sort's pieces, what both entries keep, then a group's vectors (products) or the summed
// Jacobians and, through host pointers, the staged matrix (dense).
struct Layout : SortLayout {
    int nwg = 0;
    size_t mom = 0, en = 0, part = 0, vs = 0, dmom = 0, gsum = 0, hess = 0, per_box = 0;
};

size_t base_bytes(int n, Layout& l)
{
    size_t o = 0;
    lay_sort(l, n, o);
    l.nwg = (n + kThreads - 1) / kThreads;
    l.mom = o;  o += align16(8 * (size_t)kMom * n);
    l.en = o;   o += align16(8 * (size_t)n);
    l.part = o; o += align16(8 * (size_t)kPart * l.nwg);
    return o;
}

struct Plan {
    Layout lay;
    int bpc = 0, chunks = 0, group = 0;
    size_t per_box = 0;
};

enum Mode { kMatvec, kDenseHost, kDenseDevice };

int make_plan(const char* who, int n, int nboxes, int nvec, Mode mode, size_t budget, Plan& p)
{
    Layout& l = p.lay;
    size_t o = base_bytes(n, l);
    if (mode == kMatvec) {
        const size_t per_vec = align16(24 * (size_t)n) + align16(8 * (size_t)kDm * n);
        size_t group = nvec < MW_HESS_VEC_GROUP ? nvec : MW_HESS_VEC_GROUP;
        if (budget > o && (budget - o) / per_vec < group) group = (budget - o) / per_vec;
        if (budget <= o || group < 1)
            return fail("%s: one box needs %zu bytes of scratch (nwater = %d) and does not fit the budget of %zu bytes (MW_HESS_SCRATCH_MB)", who,
                        o + per_vec, n, budget);
        p.group = (int)group;
        l.vs = o;   o += group * align16(24 * (size_t)n);
        l.dmom = o; o += group * align16(8 * (size_t)kDm * n);
    } else {
        l.gsum = o; o += align16(8 * 3 * (size_t)kDm * n);
        if (mode == kDenseHost) { l.hess = o; o += 72 * (size_t)n * n; }
    }
    l.per_box = p.per_box = o;
    const size_t fit = budget / p.per_box;
    if (fit < 1)
        return fail("%s: one box needs %zu bytes of scratch (nwater = %d%s) and does not fit the budget of %zu bytes (MW_HESS_SCRATCH_MB)", who,
                    p.per_box, n, mode == kDenseHost ? ", with its matrix of 72 nwater^2 bytes staged for the host" : "", budget);
    p.bpc = (int)(fit < (size_t)kMaxChunkBoxes ? fit : (size_t)kMaxChunkBoxes);
    if (p.bpc > nboxes) p.bpc = nboxes;
    p.chunks = (nboxes + p.bpc - 1) / p.bpc;
    return 0;
}

void hess_fields(const Plan& p, const int* grid, int* f)
{
    f[0] = p.bpc; f[1] = p.chunks; f[2] = grid[0]; f[3] = grid[1]; f[4] = grid[2];
    f[5] = kLds; f[6] = p.per_box > (size_t)INT_MAX ? INT_MAX : (int)p.per_box; f[7] = p.group;
}

int check_counts(const char* who, int nboxes, int n, int nvec, bool dense)
{
    if (nboxes < 1 || nboxes > kMaxBoxes) return fail("%s: nboxes = %d outside 1..%d", who, nboxes, kMaxBoxes);
    const int most = dense ? MW_HESS_MAX_DENSE_WATER : kMaxWater;
    if (n < 1 || n > most) return fail("%s: nwater = %d outside 1..%d", who, n, most);
    if (!dense && (nvec < 1 || nvec > MW_HESS_MAX_VEC)) return fail("%s: nvec = %d outside 1..%d", who, nvec, MW_HESS_MAX_VEC);
    return 0;
}

// Host arrays of `per_box` doubles per box: every one finite.
int check_finite(const char* who, const char* what, int nboxes, size_t per_box, const double* a)
{
    for (int b = 0; b < nboxes; ++b) {
        const double* p = a + per_box * (size_t)b;
        for (size_t k = 0; k < per_box; ++k)
            if (!std::isfinite(p[k])) return fail("%s: %s: element %zu of box %d is %g (not a finite number)", who, what, k, b, p[k]);
    }
    return 0;
}

const char kRadius[] = "a_sigma";             // the radius the cells are checked against, in the messages

int check_live(const char* who) { return check_live(who, "mw_hess_init", g); }

int add_elapsed(int a, int b, float& ms)
{
    float t = 0.0f;
    HIPOK(hipEventElapsedTime(&t, g.ev[a], g.ev[b]));
    ms += t;
    return 0;
}

// The work of the four entries, arguments and plan already checked.  par and grid are on the host; pos, vecs, out / hess and ef
// are device pointers when `dev`, host pointers otherwise.
int run(int nboxes, int n, const Plan& p, Mode mode, const std::vector<double>& par, const std::vector<int>& grid, const double* pos, bool dev,
        int nvec, const double* vecs, double* out, double* ef)
{
    const Layout& l = p.lay;
    DeviceScope scope;
    HIPOK(scope.enter(g.device));
    if (reserve(g.scratch, p.per_box * (size_t)p.bpc)) return 1;
    if (reserve(g.par, par.size() * sizeof(double))) return 1;
    if (reserve(g.grid, grid.size() * sizeof(int))) return 1;
    HIPOK(hipMemcpyAsync(g.par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, g.stream));
    HIPOK(hipMemcpyAsync(g.grid.p, grid.data(), grid.size() * sizeof(int), hipMemcpyHostToDevice, g.stream));
    const size_t vbytes = 24 * (size_t)n;                                  // one vector
    if (!dev) {
        if (reserve(g.pos, vbytes * p.bpc)) return 1;
        if (mode == kMatvec && (reserve(g.vecs, vbytes * p.group * p.bpc) || reserve(g.out, vbytes * p.group * p.bpc))) return 1;
        if (ef && reserve(g.ef, 16 * (size_t)p.bpc)) return 1;
    }
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const size_t ld = 3 * (size_t)n;
    for (int c = 0; c < p.chunks; ++c) {
        const int b0 = c * p.bpc, nb = (nboxes - b0 < p.bpc) ? nboxes - b0 : p.bpc;
        const double* d_pos = pos + 3 * (size_t)n * b0;
        if (!dev) {
            HIPOK(hipMemcpyAsync(g.pos.p, d_pos, vbytes * nb, hipMemcpyHostToDevice, g.stream));
            d_pos = (const double*)g.pos.p;
        }
        const double* d_par = (const double*)g.par.p + 18 * (size_t)b0;
        const int* d_grid = (const int*)g.grid.p + 4 * (size_t)b0;
        double* d_ef = !ef ? nullptr : dev ? ef + 2 * (size_t)b0 : (double*)g.ef.p;
        char* base = (char*)g.scratch.p;
        const size_t B = (size_t)p.bpc;
        double* mom = (double*)(base + l.mom * B);
        double* en = (double*)(base + l.en * B);
        double* part = (double*)(base + l.part * B);
        const dim3 grid_m = per_molecule(n, nb);
        Sorted s;
        HIPOK(hipEventRecord(g.ev[0], g.stream));
        if (sort_into_cells(g.stream, n, nb, l, base, B, d_par, d_grid, d_pos, s)) return 1;
        HIPOK(hipEventRecord(g.ev[1], g.stream));
        hipLaunchKernelGGL(k_hess_moments, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, mom, en);
        HIPOK(hipGetLastError());
        if (d_ef) {
            hipLaunchKernelGGL(k_hess_forces, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, (const double*)mom,
                               (const double*)en, part);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_hess_ef, dim3((unsigned)nb), dim3(64), 0, g.stream, l.nwg, (const double*)part, d_ef);
            HIPOK(hipGetLastError());
            if (!dev) HIPOK(hipMemcpyAsync(ef + 2 * (size_t)b0, g.ef.p, 16 * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
        }
        HIPOK(hipEventRecord(g.ev[2], g.stream));
        HIPOK(hipStreamSynchronize(g.stream));
        if (add_elapsed(0, 1, ms[0]) || add_elapsed(1, 2, ms[1])) return 1;
        if (mode == kMatvec) {
            double* vs = (double*)(base + l.vs * B);
            double* dmom = (double*)(base + l.dmom * B);
            for (int v0 = 0; v0 < nvec; v0 += p.group) {
                const int nv = nvec - v0 < p.group ? nvec - v0 : p.group;
                const size_t far = (size_t)nvec * 3 * n;                   // doubles from one box to the next in the caller's arrays
                const double* h_vecs = vecs + (size_t)b0 * far + (size_t)v0 * 3 * n;
                double* h_out = out + (size_t)b0 * far + (size_t)v0 * 3 * n;
                const double* d_vecs = h_vecs;
                double* d_out = h_out;
                size_t stride = far;
                if (!dev) {
                    stride = (size_t)nv * 3 * n;
                    HIPOK(hipMemcpy2DAsync(g.vecs.p, stride * 8, h_vecs, far * 8, stride * 8, (size_t)nb, hipMemcpyHostToDevice, g.stream));
                    d_vecs = (const double*)g.vecs.p;
                    d_out = (double*)g.out.p;
                }
                const dim3 grid_v(grid_m.x, (unsigned)nb, (unsigned)nv);
                HIPOK(hipEventRecord(g.ev[3], g.stream));
                hipLaunchKernelGGL(k_hess_gather, grid_v, dim3(kThreads), 0, g.stream, n, s.idx, d_vecs, stride, vs);
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_hess_dmoments, grid_v, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, (const double*)vs, dmom);
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_hess_apply, grid_v, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, s.idx, (const double*)mom,
                                   (const double*)vs, (const double*)dmom, d_out, stride);
                HIPOK(hipGetLastError());
                HIPOK(hipEventRecord(g.ev[4], g.stream));
                if (!dev) HIPOK(hipMemcpy2DAsync(h_out, far * 8, g.out.p, stride * 8, stride * 8, (size_t)nb, hipMemcpyDeviceToHost, g.stream));
                HIPOK(hipStreamSynchronize(g.stream));                     // the next group reuses the scratch and the staging buffers
                if (add_elapsed(3, 4, ms[2])) return 1;
            }
        } else {
            double* gsum = (double*)(base + l.gsum * B);
            double* d_hess = dev ? out + (size_t)b0 * ld * ld : (double*)(base + l.hess * B);
            HIPOK(hipEventRecord(g.ev[3], g.stream));
            hipLaunchKernelGGL(k_hess_jsum, grid_m, dim3(kThreads), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, gsum);
            HIPOK(hipGetLastError());
            const size_t count = ld * ld * (size_t)nb, blocks = (count / 2 + kThreads - 1) / kThreads;
            hipLaunchKernelGGL(k_hess_clear, dim3((unsigned)(blocks < kClearBlocks ? (blocks ? blocks : 1) : kClearBlocks)), dim3(kThreads), 0, g.stream, d_hess,
                               count);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_hess_rows, dim3((unsigned)n, (unsigned)nb), dim3(64), 0, g.stream, n, l.cap, d_par, d_grid, s.start, s.ss, s.idx, (const double*)mom,
                               (const double*)gsum, d_hess);
            HIPOK(hipGetLastError());
            HIPOK(hipEventRecord(g.ev[4], g.stream));
            if (!dev) HIPOK(hipMemcpyAsync(out + (size_t)b0 * ld * ld, d_hess, 8 * ld * ld * (size_t)nb, hipMemcpyDeviceToHost, g.stream));
            HIPOK(hipStreamSynchronize(g.stream));
            if (add_elapsed(3, 4, ms[3])) return 1;
        }
    }
    hess_fields(p, grid.data(), g.last);
    g.have_last = true;
    for (int k = 0; k < 4; ++k) g.ms[k] = ms[k];
    return 0;
}

// Both kinds of entry: the checks in the contract's order, then the work.
int entry(const char* who, Mode mode, bool dev, int nboxes, int n, const double* cells, const double* pos, int nvec, const double* vecs, double* out,
          const char* out_name, double* ef)
{
    std::vector<double> par;
    std::vector<int> grid;
    Plan p;
    if (check_counts(who, nboxes, n, nvec, mode != kMatvec)) return 1;
    if (!cells) return fail("%s: cells is NULL", who);
    if (!pos) return fail("%s: pos is NULL", who);
    if (mode == kMatvec && !vecs) return fail("%s: vecs is NULL", who);
    if (!out) return fail("%s: %s is NULL", who, out_name);
    if (!dev) {
        if (check_cells(who, kRadius, nboxes, n, cells, mw::kSigA, par, grid)) return 1;
        if (check_finite(who, "pos", nboxes, 3 * (size_t)n, pos)) return 1;
        if (mode == kMatvec && check_finite(who, "vecs", nboxes, 3 * (size_t)n * nvec, vecs)) return 1;
    }
    if (make_plan(who, n, nboxes, nvec, mode, g.live ? g.budget : kDefaultBudget, p)) return 1;
    if (check_live(who)) return 1;
    if (dev) {
        DeviceScope scope;
        HIPOK(scope.enter(g.device));
        if (fetch_cells(who, kRadius, nboxes, n, cells, mw::kSigA, par, grid)) return 1;
    }
    return run(nboxes, n, p, mode, par, grid, pos, dev, nvec, vecs, out, ef);
}

}  // namespace

extern "C" {

const char* mw_hess_last_error(void) { return g_err; }
int mw_hess_is_initialised(void) { return g.live ? 1 : 0; }

int mw_hess_init(int device) { return runtime_init("mw_hess_init", "MW_HESS_SCRATCH_MB", device, g); }

int mw_hess_finalize(void)
{
    if (runtime_finalize(g, {&g.scratch, &g.par, &g.grid, &g.pos, &g.vecs, &g.out, &g.ef})) return 1;
    g = State{};
    return 0;
}

int mw_hess_matvec(int nboxes, int nwater, const double* cells, const double* pos, int nvec, const double* vecs, double* out, double* ef)
{
    return entry("mw_hess_matvec", kMatvec, false, nboxes, nwater, cells, pos, nvec, vecs, out, "out", ef);
}

int mw_hess_matvec_device(int nboxes, int nwater, const double* cells, const double* pos, int nvec, const double* vecs, double* out, double* ef)
{
    return entry("mw_hess_matvec_device", kMatvec, true, nboxes, nwater, cells, pos, nvec, vecs, out, "out", ef);
}

int mw_hess_dense(int nboxes, int nwater, const double* cells, const double* pos, double* hess, double* ef)
{
    return entry("mw_hess_dense", kDenseHost, false, nboxes, nwater, cells, pos, 0, nullptr, hess, "hess", ef);
}

int mw_hess_dense_device(int nboxes, int nwater, const double* cells, const double* pos, double* hess, double* ef)
{
    return entry("mw_hess_dense_device", kDenseDevice, true, nboxes, nwater, cells, pos, 0, nullptr, hess, "hess", ef);
}

int mw_hess_plan(int nwater, const double* cell, int nboxes, int nvec, int dense, int* out, int nout)
{
    const char* who = "mw_hess_plan";
    std::vector<int> grid;
    if (check_counts(who, nboxes, nwater, nvec, dense != 0)) return 1;
    if (plan_grid(who, kRadius, nwater, cell, mw::kSigA, out, nout, grid)) return 1;
    Plan p;
    if (make_plan(who, nwater, nboxes, nvec, dense ? kDenseHost : kMatvec, g.live ? g.budget : kDefaultBudget, p)) return 1;
    int f[MW_HESS_PLAN_FIELDS];
    hess_fields(p, grid.data(), f);
    copy_fields(f, MW_HESS_PLAN_FIELDS, out, nout);
    return 0;
}

int mw_hess_last(int* out, int nout) { return last_fields("mw_hess_last", "mw_hess_init", g, g.last, MW_HESS_PLAN_FIELDS, out, nout); }

int mw_hess_elapsed_ms(float* sort, float* moments, float* apply, float* assemble)
{
    if (check_live("mw_hess_elapsed_ms")) return 1;
    if (!g.have_last) return fail("mw_hess_elapsed_ms: no call has launched yet");
    if (sort) *sort = g.ms[0];
    if (moments) *moments = g.ms[1];
    if (apply) *apply = g.ms[2];
    if (assemble) *assemble = g.ms[3];
    return 0;
}

}  // extern "C"
