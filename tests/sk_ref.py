"""Two numpy evaluations of the static structure factor, written from the definition and written differently, and the
derived bound the device (and each other) are held to.

A cell ``h`` is [3, 3] with ROW k the lattice vector h_(k+1) (bohr), positions ``xyz`` [N, 3]; s_j = xyz_j @ inv(h),
rho(n) = sum_j exp(-2 pi i n . s_j), S(n) = |rho(n)|^2 / N.

``sk_exact``: np.longdouble (64-bit mantissa on x86), the inverse cell refined by Newton steps in long double, 2 pi a
long-double literal, cos and sin of 2 pi n . s evaluated directly.  About 0.5 us per (molecule, vector): keep N M <= 1e7.
``sk_tables``: double precision through per-axis tables and complex products -- what a user can do today with numpy.
"""
import numpy as np

LD = np.longdouble
TWO_PI_LD = LD("6.283185307179586476925286766559005768394")
EPS = 2.0 ** -52


def have_extended_precision():
    return np.finfo(LD).nmant >= 63


def inverse_ld(h):
    """inv(h) in long double: the double inverse refined by Newton steps X <- X (2 - h X)."""
    hl = np.asarray(h, dtype=np.float64).astype(LD)
    x = np.linalg.inv(np.asarray(h, dtype=np.float64)).astype(LD)
    two = LD(2) * np.eye(3, dtype=LD)
    for _ in range(4):
        x = x @ (two - hl @ x)
    return x


def s_max(h, xyz):
    """max |H^-1 r| over molecules and components, positions as stored."""
    return float(np.abs(np.asarray(xyz, dtype=np.float64) @ np.linalg.inv(np.asarray(h, dtype=np.float64))).max())


def sk_exact(h, xyz, nvec, chunk=None):
    """(re, im, S) as long-double arrays [M]: rho = re + i im."""
    xyz = np.asarray(xyz, dtype=np.float64).astype(LD)
    nvec = np.asarray(nvec, dtype=np.int64)
    n, m = len(xyz), len(nvec)
    s = xyz @ inverse_ld(h)
    s = s - np.rint(s)                                   # exact in the definition: n . rint(s) is an integer
    chunk = chunk or max(1, int(2_000_000 // max(n, 1)))
    re, im = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    for a in range(0, m, chunk):
        t = s @ nvec[a:a + chunk].T.astype(LD)           # [N, c] = n . s_j
        t = t - np.rint(t)
        ph = TWO_PI_LD * t
        re[a:a + chunk] = np.cos(ph).sum(axis=0)
        im[a:a + chunk] = -np.sin(ph).sum(axis=0)
    return re, im, (re * re + im * im) / LD(n)


def sk_tables(h, xyz, nvec, chunk=None):
    """(rho complex128 [M], S float64 [M]) in double precision: per-axis tables exp(2 pi i m s_a), m = 0 .. max |n_a|, the
    conjugate entry for a negative component, the product of the three, conjugated and summed over the molecules."""
    xyz = np.asarray(xyz, dtype=np.float64)
    nvec = np.asarray(nvec, dtype=np.int64)
    n, m = len(xyz), len(nvec)
    s = xyz @ np.linalg.inv(np.asarray(h, dtype=np.float64))
    s = s - np.rint(s)
    tables = []
    for a in range(3):
        mm = np.arange(int(np.abs(nvec[:, a]).max(initial=0)) + 1, dtype=np.float64)
        ph = 2.0 * np.pi * mm[:, None] * s[None, :, a]
        tables.append(np.cos(ph) + 1j * np.sin(ph))                       # [nmax_a + 1, N]
    chunk = chunk or max(1, int(2_000_000 // max(n, 1)))
    rho = np.zeros(m, dtype=np.complex128)
    for a in range(0, m, chunk):
        nv = nvec[a:a + chunk]
        e = [np.where((nv[:, ax] < 0)[:, None], np.conj(tables[ax][np.abs(nv[:, ax])]), tables[ax][np.abs(nv[:, ax])])
             for ax in range(3)]
        rho[a:a + chunk] = np.conj((e[0] * e[1]) * e[2]).sum(axis=1)
    return rho, (rho.real ** 2 + rho.imag ** 2) / n


def delta(nvec, nwater, smax):
    """The bound on |rho - rho_exact| per vector, derived, not measured:
        delta(n) = N (8 pi eps |n|_1 max(1, s_max) + 16 eps) + eps N^2 / 2
    -- the rounding of s_j carried into the phase; three sincospi results of <= 2 ulp plus two complex products; the worst
    case of a sequential sum whose partial sums reach N."""
    l1 = np.abs(np.asarray(nvec, dtype=np.int64)).sum(axis=1).astype(np.float64)
    n = float(nwater)
    return n * (8.0 * np.pi * EPS * l1 * max(1.0, float(smax)) + 16.0 * EPS) + EPS * n * n / 2.0


def assert_within(rho, S, exact, nvec, nwater, smax, what=""):
    """|rho - rho_exact| <= delta(n) and |S - S_exact| <= (2 |rho_exact| delta + delta^2) / N for every vector; prints the
    worst ratios before it asserts."""
    re, im, s_ex = exact
    rho = np.asarray(rho)
    d = delta(nvec, nwater, smax)
    err = np.sqrt(((rho.real.astype(LD) - re) ** 2 + (rho.imag.astype(LD) - im) ** 2).astype(np.float64))
    mod = np.sqrt((re * re + im * im).astype(np.float64))
    ds = (2.0 * mod * d + d * d) / float(nwater)
    err_s = np.abs((np.asarray(S).astype(LD) - s_ex).astype(np.float64))
    print(what, "N", nwater, "M", len(d), "s_max %.3f" % smax, "max |drho| / delta %.4f" % float((err / d).max()),
          "max |dS| / bound %.4f" % float((err_s / ds).max()))
    assert np.all(err <= d), (what, int(np.argmax(err / d)), float((err / d).max()))
    assert np.all(err_s <= ds), (what, int(np.argmax(err_s / ds)), float((err_s / ds).max()))


def vectors_for(h, m_target=3500, m_cap=4096, k_cap_ang=12.0):
    """All half-space triples of the cell ``h`` up to a k_max chosen from the cell's volume so that about ``m_target`` and at
    most ``m_cap`` vectors come out (a half sphere of radius k holds V k^3 / (12 pi^2) of them)."""
    from mc_water_ls_mw_amd.structure import BOHR_TO_ANG, kvectors
    vol_ang = abs(np.linalg.det(np.asarray(h, dtype=np.float64))) * BOHR_TO_ANG ** 3
    k = min(k_cap_ang, (12.0 * np.pi ** 2 * m_target / vol_ang) ** (1.0 / 3.0))
    while True:
        nvec = kvectors(h, k, half=True)
        if len(nvec) <= m_cap:
            return nvec
        k *= 0.95
