// humanoid_math.hpp -- humanoid engine, layer 2: scalar helpers, quaternion / 3-vector / spatial-vector algebra, the contact frame and the
// nv-vector dot product.  Includes humanoid_spec.hpp.
#pragma once
#include "humanoid_spec.hpp"

namespace rex {
namespace hum {

template <class T> REX_HD T hsqrt(T a);
template <> REX_HD float hsqrt<float>(float a) { return sqrtf(a); }
template <> REX_HD double hsqrt<double>(double a) { return sqrt(a); }
template <class T> REX_HD T fast_sqrt(T a) { return hsqrt(a); }   // where a bound, not a result, is computed
#if defined(__HIP_DEVICE_COMPILE__)
template <> REX_HD float fast_sqrt<float>(float a) { return __builtin_amdgcn_sqrtf(a); }   // one v_sqrt_f32 (1 ulp), no denormal fix-up
#endif
template <class T> REX_HD T habs(T a) { return a < T(0) ? -a : a; }
template <class T> REX_HD T hmax(T a, T b) { return a > b ? a : b; }
template <class T> REX_HD T hmin(T a, T b) { return a < b ? a : b; }
REX_HD void hsincos(float a, float& s, float& c) { sincos_poly(a, s, c); }
REX_HD void hsincos(double a, double& s, double& c) { s = sin(a); c = cos(a); }

template <class T> REX_HD T dot3(const T* a, const T* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <class T> REX_HD void cross3(T* r, const T* a, const T* b) {
  T x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
template <class T> REX_HD void qmul(T* r, const T* a, const T* b) {
  T w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  T x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  T y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  T z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
template <class T> REX_HD void qnorm(T* q) {
  T n = hsqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < T(1e-15)) { q[0] = 1; q[1] = q[2] = q[3] = 0; } else { T i = rcp_t(n); q[0] *= i; q[1] *= i; q[2] *= i; q[3] *= i; }
}
template <class T> REX_HD void q2mat(T* m, const T* q) {
  T w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
template <class T> REX_HD void mulv(T* r, const T* m, const T* v) {
  T x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2], y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2], z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
// spatial motion cross product  (w;v) x (w2;v2) = (w x w2 ; w x v2 + v x w2)
template <class T> REX_HD void cross_motion(T* r, const T* a, const T* b) {
  T t1[3], t2[3], t3[3];
  cross3(t1, a, b); cross3(t2, a, b + 3); cross3(t3, a + 3, b);
  r[0] = t1[0]; r[1] = t1[1]; r[2] = t1[2]; r[3] = t2[0] + t3[0]; r[4] = t2[1] + t3[1]; r[5] = t2[2] + t3[2];
}
// spatial force cross product  (w;v) x* (n;f) = (w x n + v x f ; w x f)
template <class T> REX_HD void cross_force(T* r, const T* a, const T* f) {
  T t1[3], t2[3], t3[3];
  cross3(t1, a, f); cross3(t2, a + 3, f + 3); cross3(t3, a, f + 3);
  r[0] = t1[0] + t2[0]; r[1] = t1[1] + t2[1]; r[2] = t1[2] + t2[2]; r[3] = t3[0]; r[4] = t3[1]; r[5] = t3[2];
}
// cinert (10: Ixx Iyy Izz Ixy Ixz Iyz, m*off(3), m) times a motion vector -> force vector ([3P] mju_mulInertVec)
template <class T> REX_HD void mul_inert(T* r, const T* I, const T* v) {
  r[0] = I[0] * v[0] + I[3] * v[1] + I[4] * v[2] - I[8] * v[4] + I[7] * v[5];
  r[1] = I[3] * v[0] + I[1] * v[1] + I[5] * v[2] + I[8] * v[3] - I[6] * v[5];
  r[2] = I[4] * v[0] + I[5] * v[1] + I[2] * v[2] - I[7] * v[3] + I[6] * v[4];
  r[3] = I[8] * v[1] - I[7] * v[2] + I[9] * v[3];
  r[4] = I[6] * v[2] - I[8] * v[0] + I[9] * v[4];
  r[5] = I[7] * v[0] - I[6] * v[1] + I[9] * v[5];
}

template <class T>
REX_HD void make_frame(T* f) {   // [3P] mju_makeFrame
  const T in = rcp_t(hsqrt(dot3(f, f))); for (int k = 0; k < 3; k++) f[k] *= in;
  if (hsqrt(dot3(f + 3, f + 3)) < T(0.5)) { f[3] = f[4] = f[5] = 0; if (f[1] < T(0.5) && f[1] > T(-0.5)) f[4] = 1; else f[5] = 1; }
  T d = dot3(f, f + 3); for (int k = 0; k < 3; k++) f[3 + k] -= d * f[k];
  T n2 = hsqrt(dot3(f + 3, f + 3));
  if (n2 < T(1e-15)) { f[3] = 1; f[4] = 0; f[5] = 0; } else { const T in2 = rcp_t(n2); for (int k = 0; k < 3; k++) f[3 + k] *= in2; }
  cross3(f + 6, f, f + 3);
}

// dot product of two nv-vectors; on the device (fp32) eleven v_pk_fma_f32 + one fma instead of 23 fma
template <class T>
REX_HD T dot_nv(const T (&a)[NV], const T (&b)[NV]) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(REX_NO_PK)
  if constexpr (sizeof(T) == 4) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f acc0 = {0.0f, 0.0f}, acc1 = {0.0f, 0.0f};
    static_for<0, NV / 4>([&](auto QQ) { constexpr int q = 4 * QQ;
      acc0 = __builtin_elementwise_fma(v2f{a[q], a[q + 1]}, v2f{b[q], b[q + 1]}, acc0);
      acc1 = __builtin_elementwise_fma(v2f{a[q + 2], a[q + 3]}, v2f{b[q + 2], b[q + 3]}, acc1); });
    acc0 = __builtin_elementwise_fma(v2f{a[20], a[21]}, v2f{b[20], b[21]}, acc0);
    const v2f t = acc0 + acc1;
    return (t.x + t.y) + a[22] * b[22];
  } else
#endif
  { T r = 0; for (int k = 0; k < NV; k++) r += a[k] * b[k]; return r; }
}
static_assert(NV == 23, "dot_nv is written for nv = 23");

}  // namespace hum
}  // namespace rex
