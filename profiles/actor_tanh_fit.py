#!/usr/bin/env python3
"""Fits the coefficients of csrc/actor.hpp's tanh32 (numpy, fp64) and prints them as C constants.

    python profiles/actor_tanh_fit.py

tanh32(x), |x| < BP:   x + x^3 P(x^2), P of degree NP -- weighted least squares at Chebyshev nodes of u = x^2 on [0, BP^2], the weight
                       making the residual the RELATIVE error of tanh.
           otherwise:  1 - 2 / (e + 1), e = exp32(2 |x|) = 2^n Q(r) with n = rint(2 |x| log2 e), r = 2 |x| - n ln 2 (two constants), Q of
                       degree NQ with Q(0) = Q'(0) = 1 fixed -- least squares at Chebyshev nodes of r on [-ln 2 / 2, ln 2 / 2].
The coefficients are rounded to fp32 before the error is looked at.  The figure printed here is an estimate on a sample with fmaf emulated
through fp64; the bound the tests hold (T of include/rex.h) comes from the host twin's exhaustive sweep, tests/test_actor_host.py.
"""
import numpy as np

BP, NP, NQ = 0.625, 6, 6
F = np.float32


def cheb(lo, hi, n):
    k = np.arange(n)
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * np.cos(np.pi * (k + 0.5) / n)


def fit_tanh():
    u = cheb(0.0, BP * BP, 400)
    x = np.sqrt(u)
    target = (np.tanh(x) / x - 1.0) / u
    w = u * x / np.tanh(x)                        # residual of P times x^3 / tanh x = relative error of tanh
    A = np.vander(u, NP + 1, increasing=True)
    c, *_ = np.linalg.lstsq(A * w[:, None], target * w, rcond=None)
    return c.astype(F)


def fit_exp():
    r = cheb(-0.5 * np.log(2.0), 0.5 * np.log(2.0), 400)
    target = (np.exp(r) - 1.0 - r) / (r * r)
    A = np.vander(r, NQ - 1, increasing=True)
    c, *_ = np.linalg.lstsq(A, target, rcond=None)
    return np.concatenate([[1.0, 1.0], c]).astype(F)


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def tanh32(x, cp, cq):
    x = x.astype(F)
    a = np.abs(x)
    u = x * x
    p = np.full_like(x, cp[-1])
    for c in cp[-2::-1]:
        p = fma(p, u, np.full_like(x, c))
    small = fma(x * u, p, x)
    t = np.minimum(a, F(10.0))
    t = t + t
    n = np.rint(t * F(1.4426950408889634))
    r = fma(-n, np.full_like(x, F(0.693145751953125)), t)
    r = fma(-n, np.full_like(x, F(1.42860682030941723212e-6)), r)
    q = np.full_like(x, cq[-1])
    for c in cq[-2::-1]:
        q = fma(q, r, np.full_like(x, c))
    e = q * np.exp2(n).astype(F)
    big = np.copysign(F(1.0) - F(2.0) / (e + F(1.0)), x)
    return np.where(a < F(BP), small, big)


if __name__ == "__main__":
    cp, cq = fit_tanh(), fit_exp()
    print("constexpr float TANH_BP = %rf;" % BP)
    print("// P, degree %d in x^2, lowest first" % NP)
    print("constexpr float TANH_P[%d] = {%s};" % (NP + 1, ", ".join("%.9ef" % c for c in cp)))
    print("// Q, degree %d in r, lowest first" % NQ)
    print("constexpr float EXP_Q[%d] = {%s};" % (NQ + 1, ", ".join("%.9ef" % c for c in cq)))
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-10, 10, 2000000), rng.uniform(-1, 1, 2000000), np.nextafter(F(BP), F(0)).reshape(1), [BP]]).astype(F)
    ref = np.tanh(x.astype(np.float64))
    got = tanh32(x, cp, cq).astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(F)).astype(np.float64)
    err = np.abs(got - ref) / ulp
    k = int(np.argmax(err))
    print("// sample estimate: worst %.3f ulp at x = %r" % (err[k], float(x[k])))
    for lo, hi in ((0, BP), (BP, 1), (1, 3), (3, 10)):
        m = (np.abs(x) >= lo) & (np.abs(x) < hi)
        print("//   |x| in [%g, %g): %.3f ulp" % (lo, hi, err[m].max()))
