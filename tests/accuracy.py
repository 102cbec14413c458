"""Long-double references and the rms accuracy gate (a helper module like util.py, not a conftest).

ld_dft is a mixed-radix FFT in np.longdouble (64-bit mantissa on x86: eps 1.08e-19, about 2^11 finer than
double).  Prime factors p <= 64 are done by a direct O(p^2) butterfly, lengths with a larger prime factor by
Bluestein over a power of two.  Its own rms error is O(eps log n), so next to a double-precision FFT
(O(u log n), u = 2^-53) it is exact for every purpose here.

The metric is the rms relative error |y - Y|_2 / |Y|_2 against the long-double result Y.  The gate:

    e_gpu <= MARGIN * max(e_oracle, e_numpy, u / 2),   MARGIN = 3

Correct twiddle schemes (exact table, two-level lo * hi table, product of up to 19 binary powers) stay within
about 2.1x of a double FFT with an exact table, a table off by 4 ulp rms reaches 3.5x or more, and 10 ulp about
10x (tests/test_accuracy_ref.py pins these numbers).  The u / 2 floor covers lengths the references compute
exactly (n = 2 on inputs that are multiples of 2^-53).
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53
MARGIN = 3.0
PI = LD("3.14159265358979323846264338327950288419716939937510")

LD_REASON = None
if np.finfo(LD).nmant < 63:
    LD_REASON = "np.longdouble has %d mantissa bits here (< 63): no long-double reference" % np.finfo(LD).nmant


def require_longdouble():
    """make the calling test module skip, never pass vacuously, where long double is plain double"""
    if LD_REASON:
        import pytest
        pytest.skip(LD_REASON, allow_module_level=True)


def _check():
    if LD_REASON:
        raise RuntimeError(LD_REASON)


def _factors(n):
    f, p = [], 2
    while p * p <= n:
        while n % p == 0:
            f.append(p)
            n //= p
        p += 1
    if n > 1:
        f.append(n)
    return f


def _radices(n):
    """radices for the Stockham passes: 4s for the powers of two (one 2 if odd), then the odd primes"""
    f = _factors(n)
    twos = f.count(2)
    out = [4] * (twos // 2) + [2] * (twos % 2)
    return out + [p for p in f if p != 2]


_ROOTS = {}


def _roots(n, sign):
    """exp(sign 2 pi i j / n), j < n, long double, cached per (n, sign)"""
    key = (n, sign)
    if key not in _ROOTS:
        if len(_ROOTS) > 8:
            _ROOTS.clear()
        j = np.arange(n, dtype=np.int64)
        ang = (2 * PI) * j.astype(LD) / LD(n)
        _ROOTS[key] = np.cos(ang) + (1j * sign) * np.sin(ang).astype(CLD)
    return _ROOTS[key]


def _stockham(x, sign, radices, roots, N):
    """x: (B, n) clongdouble, n = prod(radices); roots: exp(sign 2 pi i j / N), n | N.
    Decimation in time: the p sub-sequences x[r::p] first, then twiddles w_n^(r k2) and p-point DFTs."""
    B, n = x.shape
    if n == 1:
        return x.copy()
    p = radices[0]
    m = n // p
    S = _stockham(np.ascontiguousarray(x.reshape(B, m, p).transpose(0, 2, 1)).reshape(B * p, m),
                  sign, radices[1:], roots, N).reshape(B, p, m)
    if m > 1:
        r = np.arange(1, p, dtype=np.int64)[:, None]
        k2 = np.arange(m, dtype=np.int64)[None, :]
        S[:, 1:, :] *= roots[(r * k2) * (N // n)]
    out = np.empty((B, p, m), dtype=CLD)
    if p == 2:
        np.add(S[:, 0], S[:, 1], out=out[:, 0])
        np.subtract(S[:, 0], S[:, 1], out=out[:, 1])
    elif p == 4:
        a, b, c, d = S[:, 0], S[:, 1], S[:, 2], S[:, 3]
        s0, s1 = a + c, a - c
        t0 = b + d
        t1 = (b - d) * CLD(1j * sign)          # exact: a swap and a sign
        out[:, 0] = s0 + t0
        out[:, 2] = s0 - t0
        out[:, 1] = s1 + t1
        out[:, 3] = s1 - t1
    else:
        W = roots[(np.arange(p, dtype=np.int64) * (N // p)) % N]
        for k1 in range(p):
            acc = S[:, 0].copy()
            for r in range(1, p):
                acc += W[(k1 * r) % p] * S[:, r]
            out[:, k1] = acc
    return out.reshape(B, n)


def _fft_rows(x, sign, force_bluestein=False):
    """1-D DFT of every row of x (B, n), long double"""
    _check()
    B, n = x.shape
    if n == 1:
        return x.astype(CLD)
    if force_bluestein or max(_factors(n)) > 64:
        return _bluestein_rows(x, sign)
    return _stockham(np.asarray(x, dtype=CLD), sign, _radices(n), _roots(n, sign), n)


def _bluestein_rows(x, sign):
    """X[k] = c[k] sum_j (x[j] c[j]) conj(c[k - j]), c[k] = exp(sign i pi k^2 / n), k^2 reduced mod 2n in int64;
    the convolution by long-double FFTs of the power of two M >= 2n - 1"""
    B, n = x.shape
    M = 1
    while M < 2 * n - 1:
        M *= 2
    k = np.arange(n, dtype=np.int64)
    q = (k * k) % (2 * n)
    ang = PI * q.astype(LD) / LD(n)
    c = np.cos(ang) + (1j * sign) * np.sin(ang).astype(CLD)
    a = np.zeros((B, M), dtype=CLD)
    a[:, :n] = np.asarray(x, dtype=CLD) * c
    b = np.zeros((1, M), dtype=CLD)
    b[0, :n] = np.conj(c)
    b[0, M - n + 1:] = np.conj(c[1:][::-1])
    rad = _radices(M)
    A = _stockham(a, -1, rad, _roots(M, -1), M)
    Bk = _stockham(b, -1, rad, _roots(M, -1), M)
    conv = _stockham(A * Bk, +1, rad, _roots(M, +1), M) / LD(M)
    return conv[:, :n] * c


def ld_dft(x, shape, howmany=1, sign=-1, force_bluestein=False):
    """unnormalised DFT (sign -1 forward, +1 backward) of `howmany` contiguous transforms of `shape`,
    long double; N-D axis by axis.  Returns clongdouble of shape (howmany,) + shape."""
    shape = tuple(int(s) for s in shape)
    y = np.array(np.asarray(x).reshape((howmany,) + shape), dtype=CLD)
    for ax in range(1, len(shape) + 1):
        z = np.moveaxis(y, ax, -1)
        zs = z.shape
        z = _fft_rows(np.ascontiguousarray(z).reshape(-1, zs[-1]), sign, force_bluestein)
        y = np.moveaxis(z.reshape(zs), -1, ax)
    return np.ascontiguousarray(y)


def ld_r2c(x, n, howmany=1):
    """the first n // 2 + 1 outputs of the forward complex DFT of the real rows x (howmany, n)"""
    y = ld_dft(np.asarray(x, dtype=LD).reshape(howmany, n), (n,), howmany, -1)
    return np.ascontiguousarray(y[:, :n // 2 + 1])


def ld_c2r(Y, n, howmany=1):
    """unnormalised inverse of the Hermitian extension of the half spectra Y (howmany, n // 2 + 1); like FFTW's
    c2r it ignores the imaginary parts of Y[0] and, for even n, of Y[n / 2]"""
    h = n // 2 + 1
    Y = np.array(np.asarray(Y).reshape(howmany, h), dtype=CLD)
    Y[:, 0] = Y[:, 0].real
    if n % 2 == 0:
        Y[:, n // 2] = Y[:, n // 2].real
    full = np.zeros((howmany, n), dtype=CLD)
    full[:, :h] = Y
    k = np.arange(h, n)
    full[:, k] = np.conj(Y[:, n - k])
    return ld_dft(full, (n,), howmany, +1).real


def _cs(num, den, fn):
    """cos / sin(pi num / den), the integer angle reduced mod 2 den first"""
    m = np.asarray(num, dtype=np.int64) % (2 * den)
    return fn(PI * m.astype(LD) / LD(den))


def ld_r2r(x, kind):
    """the eleven r2r kinds by their defining sums (FFTW manual, "What FFTW Really Computes"), long double,
    unnormalised, for n <= 4096.  kind = FFTW's enum: R2HC 0, HC2R 1, DHT 2, REDFT00 3, REDFT01 4, REDFT10 5,
    REDFT11 6, RODFT00 7, RODFT01 8, RODFT10 9, RODFT11 10.  x: (n,) or (howmany, n); the rows of a batch share
    each block of the cosine / sine matrix, and every row is summed as it would be alone."""
    _check()
    x = np.asarray(x, dtype=LD)
    if x.ndim == 1:
        return ld_r2r(x[None, :], kind)[0]
    n = x.shape[1]
    assert n <= 4096
    j = np.arange(n, dtype=np.int64)[None, :]
    out = np.empty(x.shape, dtype=LD)
    blk = max(1, (1 << 20) // n)
    for k0 in range(0, n, blk):
        k = np.arange(k0, min(n, k0 + blk), dtype=np.int64)[:, None]
        sgn = np.where(k[:, 0] % 2 == 0, LD(1), LD(-1))
        if kind == 0:          # R2HC: r0 ... r(n/2), i((n+1)/2 - 1) ... i1
            q = np.where(k <= n // 2, k, n - k)
            c, s, low = _cs(2 * j * q, n, np.cos), _cs(2 * j * q, n, np.sin), k[:, 0] <= n // 2
            f = lambda r: np.where(low, np.sum(r * c, axis=1), -np.sum(r * s, axis=1))
        elif kind == 1:        # HC2R: x0 + 2 sum (r_q cos - i_q sin) (+ r(n/2) (-1)^k for even n)
            q = np.arange(1, (n + 1) // 2, dtype=np.int64)[None, :]
            c, s = _cs(2 * q * k, n, np.cos), _cs(2 * q * k, n, np.sin)
            if n % 2 == 0:
                f = lambda r: r[0] + 2 * np.sum(r[1:(n + 1) // 2] * c - r[n - q[0]] * s, axis=1) + sgn * r[n // 2]
            else:
                f = lambda r: r[0] + 2 * np.sum(r[1:(n + 1) // 2] * c - r[n - q[0]] * s, axis=1)
        elif kind == 2:        # DHT
            c = _cs(2 * j * k, n, np.cos) + _cs(2 * j * k, n, np.sin)
            f = lambda r: np.sum(r * c, axis=1)
        elif kind == 3:        # REDFT00, logical N = 2(n - 1)
            if n > 2:
                c = _cs(j[:, 1:n - 1] * k, n - 1, np.cos)
                f = lambda r: r[0] + sgn * r[n - 1] + 2 * np.sum(r[1:n - 1] * c, axis=1)
            else:
                f = lambda r: r[0] + sgn * r[n - 1]
        elif kind == 4:        # REDFT01
            c = _cs(j[:, 1:] * (2 * k + 1), 2 * n, np.cos)
            f = lambda r: r[0] + 2 * np.sum(r[1:] * c, axis=1)
        elif kind == 8:        # RODFT01
            c = _cs((j[:, :n - 1] + 1) * (2 * k + 1), 2 * n, np.sin)
            f = lambda r: sgn * r[n - 1] + 2 * np.sum(r[:n - 1] * c, axis=1)
        else:
            if kind == 5:      # REDFT10
                c = _cs((2 * j + 1) * k, 2 * n, np.cos)
            elif kind == 6:    # REDFT11
                c = _cs((2 * j + 1) * (2 * k + 1), 4 * n, np.cos)
            elif kind == 7:    # RODFT00, logical N = 2(n + 1)
                c = _cs((j + 1) * (k + 1), n + 1, np.sin)
            elif kind == 9:    # RODFT10
                c = _cs((2 * j + 1) * (k + 1), 2 * n, np.sin)
            elif kind == 10:   # RODFT11
                c = _cs((2 * j + 1) * (2 * k + 1), 4 * n, np.sin)
            else:
                raise ValueError(kind)
            f = lambda r: 2 * np.sum(r * c, axis=1)
        for b in range(x.shape[0]):
            out[b, k0:k0 + k.shape[0]] = f(x[b])
    return out


def rms_err(got, ref):
    """rms relative error |got - ref|_2 / |ref|_2, computed in long double"""
    got = np.asarray(got).reshape(-1)
    ref = np.asarray(ref).reshape(-1)
    assert got.size == ref.size
    if np.iscomplexobj(got) or np.iscomplexobj(ref):
        g, r = got.astype(CLD), ref.astype(CLD)
        d = g - r
        num = np.sum(d.real * d.real + d.imag * d.imag)
        den = np.sum(r.real * r.real + r.imag * r.imag)
    else:
        g, r = got.astype(LD), ref.astype(LD)
        num = np.sum((g - r) ** 2)
        den = np.sum(r * r)
    assert np.isfinite(num) and den > 0
    return float(np.sqrt(num / den))


def rms_err_per_transform(got, ref, howmany):
    """rms_err of every batch entry on its own: the arrays are (howmany, ...) in any flat layout"""
    got = np.asarray(got).reshape(howmany, -1)
    ref = np.asarray(ref).reshape(howmany, -1)
    return np.array([rms_err(got[b], ref[b]) for b in range(howmany)])


def bound(*e_refs):
    """the gate's right-hand side: MARGIN * max(references, u / 2)"""
    return MARGIN * max(max(e_refs), U / 2)


def passes(e, *e_refs):
    return e <= bound(*e_refs)
