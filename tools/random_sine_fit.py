#!/usr/bin/env python3
"""Coefficients and error bound of random()'s short sine (lt_device.hpp: random_fast_r).

    sin(m) = m (1 + z g(z)),  z = m^2,  g(z) = sum_k (-1)^(k+1) z^k / (2k + 3)!        for 0 <= m <= pi / 2

q is the polynomial of degree DEG that interpolates g in the Chebyshev points of [0, ZMAX] (ZMAX a little past (pi / 2)^2),
its coefficients rounded to double.  What is printed:

  * the coefficients as C hexadecimal literals;
  * the interpolation remainder, PROVED:  |g - q_exact| <= max |g^(n)| / n! * 2 (ZMAX / 4)^n with n = DEG + 1, and g^(n) is an
    alternating series of decreasing terms whose first is n! / (2n + 3)!;  in units of sin(m) it is multiplied by
    W = max z m / sin(m) = ZMAX^(3/2) / sin(sqrt(ZMAX));
  * what rounding the coefficients adds, PROVED:  u sum |c_k| ZMAX^k W;
  * the same two together MEASURED on a grid in 60-digit arithmetic (a check of the above, not part of the bound);
  * the running error bound of the evaluation in double precision (the operation sequence of random_fast_r), in units of
    u = 2^-53, and the sum delta' that the comment in front of random_fast_r states.

Run:  python3 tools/random_sine_fit.py        (needs mpmath)"""
import struct

from mpmath import mp, mpf, sin, cos, sqrt, pi, factorial, matrix, lu_solve

mp.dps = 60
DEG = 7
ZMAX = mpf("2.4675")     # (pi / 2)^2 = 2.46740110...
U = mpf(2) ** -53
K = mpf(struct.unpack("<d", struct.pack("<d", 43758.5453))[0])


def g(z):
    if z < mpf(10) ** -12:
        return -mpf(1) / 6 + z / 120
    m = sqrt(z)
    return (sin(m) / m - 1) / z


def to_double(x):
    return struct.unpack("<d", struct.pack("<d", float(x)))[0]


n = DEG + 1
nodes = [ZMAX / 2 * (1 + cos(pi * (2 * i + 1) / (2 * n))) for i in range(n)]
A = matrix(n, n)
b = matrix(n, 1)
for i, z in enumerate(nodes):
    for k in range(n):
        A[i, k] = z ** k
    b[i] = g(z)
exact = lu_solve(A, b)
coef = [to_double(exact[k]) for k in range(n)]

print("// q(z), degree %d, Chebyshev interpolant of (sin(sqrt z) / sqrt z - 1) / z on [0, %s]" % (DEG, ZMAX))
for k, c in enumerate(coef):
    print("  c%d = %s   // %.17g" % (k, float.hex(c), c))

W = ZMAX ** mpf("1.5") / sin(sqrt(ZMAX))
remainder = factorial(n) / factorial(2 * n + 3) / factorial(n) * 2 * (ZMAX / 4) ** n * W
rounding = U * sum(abs(mpf(c)) * ZMAX ** k for k, c in enumerate(coef)) * W
print("interpolation remainder, relative to sin(m):  %.3e = %.3f u   (proved)" % (remainder, remainder / U))
print("rounding of the coefficients:                  %.3e = %.3f u   (proved)" % (rounding, rounding / U))

worst = mpf(0)
N = 20000
for i in range(1, N + 1):
    z = ZMAX * i / N
    m = sqrt(z)
    q = mpf(0)
    for c in reversed(coef):
        q = q * z + mpf(c)
    worst = max(worst, abs(m * (1 + z * q) - sin(m)) / sin(m))
print("both, measured on %d points:                %.3e = %.3f u" % (N, worst, worst / U))

# The evaluation in double precision, every operation rounded once (fma counts as one):
#   z = m * m;  h = c7;  h = fma(h, z, c_k) for k = 6 .. 0;  t = h * z;  s = fma(t, m, m);  p = s * K
# Running error bound at z = ZMAX (every term grows with z):  the error of h after step k is at most
#   e_k = e_(k+1) z (1 + u) + u |h_k|   and z itself is off by u z, which moves q by at most u z |q'(z)|.
z = ZMAX
e = mpf(0)
h = abs(mpf(coef[-1]))
for c in reversed(coef[:-1]):
    h = h * z + abs(mpf(c))            # (a bound of |h_k| by the sum of magnitudes)
    e = e * z * (1 + U) + U * h * (1 + U)
qprime = sum(k * abs(mpf(c)) * z ** (k - 1) for k, c in enumerate(coef) if k)
e_q = e + U * z * qprime
t_abs = z * h
e_t = z * (1 + U) * e_q + 2 * U * t_abs * (1 + U)     # z's own error and the product's rounding
one_plus_T = sin(sqrt(ZMAX)) / sqrt(ZMAX)             # 1 + T >= this: the relative weight of t's error in s
e_s = e_t / one_plus_T + U                            # ... and the fma's rounding
print("evaluation: |q^ - q| <= %.3f u, |t^ - t| <= %.3f u, s relative <= %.3f u" % (e_q / U, e_t / U, e_s / U))
reflect = U * (1 + mpf("0.23"))                       # m = fl((pi_hi - |r|) + pi_lo): one rounding, pi_lo's own below 0.23 u m
poly = remainder + rounding
fast = poly + e_s + reflect + U                       # ... + the product by K
library = 4 * 2 * U + U                               # 4 ulp of a sine (one ulp is at most 2 u of the value) + its product
total = (fast + library) * (1 + mpf(2) ** -40)
print("p~ against sin(r) K:        %.3f u = 2^%.2f" % (fast / U, mp.log(fast, 2)))
print("library against sin(r) K:   %.3f u" % (library / U))
print("p~ against the library's:   %.3f u = 2^%.2f   (delta' of the CLAIM)" % (total / U, mp.log(total, 2)))
delta = mpf(2) ** -46
print("delta = 2^-46 = %.0f u;  needed: delta' (1 + delta) + u (1 + delta) = %.3f u" % (delta / U, (total * (1 + delta) + U * (1 + delta)) / U))
print("fallback rate per lane at most 2 delta 2^24 = 2^%.0f" % mp.log(2 * delta * 2 ** 24, 2))
pi_hi = mpf(to_double(pi))
print("pi_hi = %s, pi_lo = %s" % (float.hex(float(pi_hi)), float.hex(to_double(pi - pi_hi))))
