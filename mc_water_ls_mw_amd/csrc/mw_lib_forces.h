// The force layer the inherent-structure quenches and the molecular dynamics (mw_md.hip, mw_npt.hip) share: a molecule's
// moments and energy (Sums), the derivative of its triplet sum against a centre's moments (triplet_grad), the force one entry
// puts on it (entry_force), that entry's share of the scalar virial (entry_virial, used by mw_npt.hip alone) and of the virial
// tensor (entry_stress, used by mw_flex.hip alone), the cell held
// in vector registers (CellRegs / in_vgpr) and the reductions in a fixed order (the DPP trees of a wavefront, block_reduce over
// the wavefronts of a workgroup).  Device code only, all of it inlined: every library
// compiles it into its own kernels and exports nothing from here.  Included after `#pragma clang fp contract(off)`, after
// mw_common.hip.h and after mw_lib_cells.h (block_reduce is written for its kThreads).  The derivatives are those of
// mw_forces.hip.h, written again here: these libraries share mw_common.hip.h with the engine and nothing else.
#pragma once

namespace mwforces {

constexpr int kMom = mw::kMomStride;              // S0, S1 (3), S2 (xx, yy, xy, xz, yz), the number of entries
constexpr double kAepsBSig4 = mw::kAeps * mw::kBigB * mw::kSigSq * mw::kSigSq;   // A eps B sigma^4
constexpr double kOneMinusCos0Sq = (1.0 - mw::kCos0) * (1.0 - mw::kCos0);
constexpr double kCos0Sq = mw::kCos0 * mw::kCos0;

// ---- the energy of a molecule and its moments ------------------------------------------------------------------------------
// add(): the entry at d with |d|^2 = r2 < (a sigma)^2.
struct Sums {
    double e2 = 0.0, Q = 0.0, S0 = 0.0, S1x = 0.0, S1y = 0.0, S1z = 0.0;
    double Sxx = 0.0, Syy = 0.0, Szz = 0.0, Sxy = 0.0, Sxz = 0.0, Syz = 0.0;
    int cnt = 0;
    __device__ __forceinline__ void add(double r2, double dx, double dy, double dz)
    {
        double rinv, e1, g;
        mw::pair_terms(r2, rinv, e1, g);
        const double ri2 = rinv * rinv, ri4 = ri2 * ri2;
        e2 = __builtin_fma(__builtin_fma(ri4, kAepsBSig4, -mw::kAeps), e1, e2);       // A eps (B (sigma / r)^4 - 1) e1
        const double w1 = g * rinv, w2 = g * ri2;
        const double hx = w2 * dx, hy = w2 * dy, hz = w2 * dz;
        S0 = S0 + g;
        Q = __builtin_fma(g, g, Q);
        S1x = __builtin_fma(w1, dx, S1x); S1y = __builtin_fma(w1, dy, S1y); S1z = __builtin_fma(w1, dz, S1z);
        Sxx = __builtin_fma(hx, dx, Sxx); Syy = __builtin_fma(hy, dy, Syy); Szz = __builtin_fma(hz, dz, Szz);
        Sxy = __builtin_fma(hx, dy, Sxy); Sxz = __builtin_fma(hx, dz, Sxz); Syz = __builtin_fma(hy, dz, Syz);
        ++cnt;
    }
    // 1/2 sum phi + lambda eps T,  T = 1/2 [ (|S2|^2 - Q) - 2 c0 (|S1|^2 - Q) + c0^2 (S0^2 - Q) ],  Q = sum g^2
    __device__ __forceinline__ double energy() const
    {
        const double D2 = __builtin_fma(Szz, Szz, __builtin_fma(Syy, Syy, Sxx * Sxx));
        const double O2 = __builtin_fma(Syz, Syz, __builtin_fma(Sxz, Sxz, Sxy * Sxy));
        const double F2 = __builtin_fma(2.0, O2, D2);
        const double F1 = __builtin_fma(S1z, S1z, __builtin_fma(S1y, S1y, S1x * S1x));
        const double A = F2 - Q, B = F1 - Q, C = __builtin_fma(S0, S0, -Q);
        const double T = 0.5 * __builtin_fma(kCos0Sq, C, __builtin_fma(-2.0 * mw::kCos0, B, A));
        return __builtin_fma(0.5, e2, mw::kLamEps * T);
    }
    __device__ __forceinline__ void record(double (&M)[kMom]) const
    {
        M[0] = S0; M[1] = S1x; M[2] = S1y; M[3] = S1z; M[4] = Sxx; M[5] = Syy; M[6] = Sxy; M[7] = Sxz; M[8] = Syz; M[9] = (double)cnt;
    }
};

// dT / dd of an entry with unit vector u, 1 / r, g and g' against the moments M of a centre: SIGN = -1 the molecule's own
// triplets, SIGN = +1 (and the result's sign flipped, d' = -d) those centred on the neighbour, seen from the arm.
//   P = u^T S2 u + 2 s c0 u.S1 + c0^2 S0 - g (1 - c0)^2,  v = S2 u + s c0 S1,  t = P g' u + 2 g (v - (u.v) u) / r
template <int SIGN>
__device__ __forceinline__ void triplet_grad(const double (&M)[kMom], double ux, double uy, double uz, double rinv, double g, double dg,
                                             double& tx, double& ty, double& tz)
{
    constexpr double sc = SIGN * mw::kCos0;
    const double Szz = (M[0] - M[4]) - M[5];                           // the u_k are unit vectors
    const double ax = __builtin_fma(M[4], ux, __builtin_fma(M[6], uy, M[7] * uz));
    const double ay = __builtin_fma(M[6], ux, __builtin_fma(M[5], uy, M[8] * uz));
    const double az = __builtin_fma(M[7], ux, __builtin_fma(M[8], uy, Szz * uz));
    const double uS1 = __builtin_fma(M[1], ux, __builtin_fma(M[2], uy, M[3] * uz));
    const double uau = __builtin_fma(ux, ax, __builtin_fma(uy, ay, uz * az));
    const double P = __builtin_fma(-g, kOneMinusCos0Sq, __builtin_fma(kCos0Sq, M[0], __builtin_fma(2.0 * sc, uS1, uau)));
    const double vx = __builtin_fma(sc, M[1], ax), vy = __builtin_fma(sc, M[2], ay), vz = __builtin_fma(sc, M[3], az);
    const double uv = __builtin_fma(ux, vx, __builtin_fma(uy, vy, uz * vz));
    const double c = 2.0 * g * rinv, p = P * dg;
    tx = __builtin_fma(p, ux, c * __builtin_fma(-uv, ux, vx));
    ty = __builtin_fma(p, uy, c * __builtin_fma(-uv, uy, vy));
    tz = __builtin_fma(p, uz, c * __builtin_fma(-uv, uz, vz));
}

// The force the entry at d puts on the molecule with the moments Mi; Mj are the moments of the entry's molecule.
// phi = A eps (B sigma^4 r^-4 - 1) e1: phi' = -e1 [4 A eps B sigma^4 r^-5 + A eps (B sigma^4 r^-4 - 1) sigma / D^2], g' = -gamma sigma g / D^2,
// D = r - a sigma clamped as in pair_terms (past the clamp e1 = g = 0 and both derivatives are exactly 0).
__device__ __forceinline__ void entry_force(const double (&Mi)[kMom], const double (&Mj)[kMom], double r2, double dx, double dy, double dz,
                                            double& fx, double& fy, double& fz)
{
    double rinv, e1, g;
    mw::pair_terms(r2, rinv, e1, g);
    const double w = mw::fast_rcp(__builtin_fmin(__builtin_fma(r2, rinv, -mw::kSigA), mw::kDenClamp));
    const double w2 = w * w, ri2 = rinv * rinv, ri4 = ri2 * ri2;
    const double dphi = -e1 * __builtin_fma(4.0 * kAepsBSig4 * ri4, rinv, __builtin_fma(ri4, kAepsBSig4, -mw::kAeps) * (mw::kSigma * w2));
    const double dg = -mw::kGamSig * g * w2;
    const double ux = dx * rinv, uy = dy * rinv, uz = dz * rinv;
    double tx, ty, tz, sx, sy, sz;
    triplet_grad<-1>(Mi, ux, uy, uz, rinv, g, dg, tx, ty, tz);
    triplet_grad<1>(Mj, ux, uy, uz, rinv, g, dg, sx, sy, sz);
    fx = fx + __builtin_fma(mw::kLamEps, tx + sx, dphi * ux);
    fy = fy + __builtin_fma(mw::kLamEps, ty + sy, dphi * uy);
    fz = fz + __builtin_fma(mw::kLamEps, tz + sz, dphi * uz);
}

// entry_force, and the entry's share of the scalar virial W = tr of the engine's virial = -3 V dE/dV (mw_energy.h; the pressure
// is (2 K + W) / (3 V)).  e, the force of this entry alone, is entry_force's term from zeroed sums, so f gets the bits entry_force
// gives it; dw = dw + d . e.  Every pair (i, entry k) has its mirror (j, entry -d), and e holds both the derivative of the centre's
// own energy against d and that of the neighbour's against -d, so the sum of d . e over all entries of a box counts every
// d . dE/dd twice with the sign of a force: W of the box = -1/2 the sum of the lanes' dw (lane_virial), each lane in the order of
// its walk.  An image of the molecule itself is skipped by the walks' callers: the cell rule keeps it beyond the cutoff.
__device__ __forceinline__ void entry_virial(const double (&Mi)[kMom], const double (&Mj)[kMom], double r2, double dx, double dy, double dz,
                                             double& fx, double& fy, double& fz, double& dw)
{
    double ex = 0.0, ey = 0.0, ez = 0.0;
    entry_force(Mi, Mj, r2, dx, dy, dz, ex, ey, ez);
    fx = fx + ex; fy = fy + ey; fz = fz + ez;
    dw = dw + __builtin_fma(dx, ex, __builtin_fma(dy, ey, dz * ez));
}
__device__ __forceinline__ double lane_virial(double dw) { return -0.5 * dw; }

// entry_virial, and the entry's share of the virial tensor (mw_flex.hip alone): f and dw get the bits entry_virial gives them;
// s holds the lane's sums in the order xx, yy, zz, xy, xz, yz, s_aa = fma(d_a, e_a, s_aa) and, symmetrised,
// s_ab = s_ab + fma(d_a, e_b, d_b e_a).  Every pair is visited from both ends as for W, and an off-diagonal sum counts d_a e_b and
// d_b e_a both: the lane's share of W_ab is -1/2 s on the diagonal and -1/4 s off it (lane_stress).
__device__ __forceinline__ void entry_stress(const double (&Mi)[kMom], const double (&Mj)[kMom], double r2, double dx, double dy, double dz,
                                             double& fx, double& fy, double& fz, double& dw, double (&s)[6])
{
    double ex = 0.0, ey = 0.0, ez = 0.0;
    entry_force(Mi, Mj, r2, dx, dy, dz, ex, ey, ez);
    fx = fx + ex; fy = fy + ey; fz = fz + ez;
    dw = dw + __builtin_fma(dx, ex, __builtin_fma(dy, ey, dz * ez));
    s[0] = __builtin_fma(dx, ex, s[0]); s[1] = __builtin_fma(dy, ey, s[1]); s[2] = __builtin_fma(dz, ez, s[2]);
    s[3] = s[3] + __builtin_fma(dx, ey, dy * ex);
    s[4] = s[4] + __builtin_fma(dx, ez, dz * ex);
    s[5] = s[5] + __builtin_fma(dy, ez, dz * ey);
}
__device__ __forceinline__ double lane_stress(double s, int k) { return k < 3 ? -0.5 * s : -0.25 * s; }

// The cell's nine doubles held in vector registers.  Left to itself the compiler keeps them in 18 scalar registers next to the
// scalar constants of pair_terms' polynomial, and the walks of the force pass then run out of scalar registers and spill.
__device__ __forceinline__ double in_vgpr(double t)
{
    asm("" : "+v"(t));
    return t;
}
struct CellRegs {
    double c[9];
    __device__ __forceinline__ explicit CellRegs(const double* __restrict__ H)
    {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            c[k] = in_vgpr(H[k]);
        }
    }
};

// ---- reductions in a fixed order ---------------------------------------------------------------------------------------------
// the largest of 64 non-negative values through the DPP network of mw::dpp_wave_min; lane 63 ends up with it
__device__ __forceinline__ double dpp_wave_max(double v)
{
    double o;
    o = mw::dpp_keep_f64<0x111, 0xf>(v); v = o > v ? o : v;
    o = mw::dpp_keep_f64<0x112, 0xf>(v); v = o > v ? o : v;
    o = mw::dpp_keep_f64<0x114, 0xf>(v); v = o > v ? o : v;
    o = mw::dpp_keep_f64<0x118, 0xf>(v); v = o > v ? o : v;
    o = mw::dpp_keep_f64<0x142, 0xa>(v); v = o > v ? o : v;
    o = mw::dpp_keep_f64<0x143, 0xc>(v); v = o > v ? o : v;
    return v;
}
__device__ __forceinline__ double wave_total(double v) { return mw::readlane_f64(mw::dpp_wave_sum(v), 63); }
__device__ __forceinline__ double wave_largest(double v) { return mw::readlane_f64(dpp_wave_max(v), 63); }

// NS sums and then NM maxima of a workgroup of kThreads: the lanes of a wavefront by the DPP tree, the wavefronts in order.
// Thread k < NS + NM returns value k; every thread calls this, and it holds two barriers.
template <int NS, int NM>
__device__ __forceinline__ double block_reduce(const double (&val)[NS + NM], double (*red)[NS + NM])
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    __syncthreads();                                                   // (red may still be read from an earlier call)
#pragma unroll
    for (int k = 0; k < NS + NM; ++k) {
        const double w = k < NS ? mw::dpp_wave_sum(val[k]) : dpp_wave_max(val[k]);
        if (lane == 63) red[wid][k] = w;
    }
    __syncthreads();
    double out = 0.0;
    if (tid < NS + NM) {
        out = red[0][tid];
        for (int w = 1; w < mwcells::kThreads / 64; ++w) out = tid < NS ? out + red[w][tid] : (red[w][tid] > out ? red[w][tid] : out);
    }
    return out;
}

}  // namespace mwforces
