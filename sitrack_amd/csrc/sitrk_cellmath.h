// sitrk_cellmath.h -- the per-cell arithmetic of two contracts of include/sitrk.h as __device__ functions, so that every kernel
// that evaluates them runs the same statements: the deformation rates of sitrk_deform_cells and the shoelace
// sum, acceptance tests and score of sitrk_tri2quad.  Included by sitrk_deform.hip, sitrk_quadmesh.hip,
// sitrk_mesh.hip, sitrk_raster.hip and sitrk_coarse.hip only; one rounded fp64 operation per symbol, no fused multiply-add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double plus_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ bool finite64(double a) { return fabs(a) < plus_inf(); }

// The contract of sitrk_deform_cells on one cell: a = its vertices at t0, b = at t1, T seconds apart.  r = div, shr, vor, area0,
// area1 as computed; false: the cell is invalid (a coordinate not finite, A2 zero or not finite) and r is not to be used.
template <int NV>
__device__ __forceinline__ bool deform_rates(const pt (&a)[NV], const pt (&b)[NV], double T, double (&r)[5])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NV; k++) ok = ok && finite64(a[k].y) && finite64(a[k].x) && finite64(b[k].y) && finite64(b[k].x);

    double dx[NV], dy[NV], ex[NV], ey[NV], u[NV], v[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        dx[k] = a[k].x - a[0].x; dy[k] = a[k].y - a[0].y;
        ex[k] = b[k].x - b[0].x; ey[k] = b[k].y - b[0].y;
        u[k] = (b[k].x - a[k].x) / T; v[k] = (b[k].y - a[k].y) / T;
    }
    double A2 = 0.0, B2 = 0.0, Suy = 0.0, Sux = 0.0, Svy = 0.0, Svx = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int q = (k + 1) % NV;
        A2 = A2 + (dx[k] * dy[q] - dx[q] * dy[k]);
        B2 = B2 + (ex[k] * ey[q] - ex[q] * ey[k]);
        const double us = u[q] + u[k], vs = v[q] + v[k], ddy = dy[q] - dy[k], ddx = dx[q] - dx[k];
        Suy = Suy + us * ddy; Sux = Sux + us * ddx;
        Svy = Svy + vs * ddy; Svx = Svx + vs * ddx;
    }
    ok = ok && A2 != 0.0 && finite64(A2);
    const double ux = Suy / A2, uy = -(Sux / A2), vx = Svy / A2, vy = -(Svx / A2);
    const double e1 = ux - vy, e2 = uy + vx;
    r[0] = ux + vy;
    r[1] = sqrt(e1 * e1 + e2 * e2);
    r[2] = vx - uy;
    r[3] = 0.5 * fabs(A2);
    r[4] = 0.5 * fabs(B2);
    return ok;
}

// The velocity gradients of the same contract, for the box averages of sitrk_coarse_* (DESIGN.md 3.16): the statements of
// deform_rates up to u_x, u_y, v_x, v_y, in the same order, so that both give the same bits for them.  g = a, a*u_x, a*u_y, a*v_x,
// a*v_y with a = area0; false: the cell is invalid in the sense of deform_rates and g is not to be used.
template <int NV>
__device__ __forceinline__ bool deform_gradient_terms(const pt (&a)[NV], const pt (&b)[NV], double T, double (&g)[5])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < NV; k++) ok = ok && finite64(a[k].y) && finite64(a[k].x) && finite64(b[k].y) && finite64(b[k].x);

    double dx[NV], dy[NV], u[NV], v[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) {
        dx[k] = a[k].x - a[0].x; dy[k] = a[k].y - a[0].y;
        u[k] = (b[k].x - a[k].x) / T; v[k] = (b[k].y - a[k].y) / T;
    }
    double A2 = 0.0, Suy = 0.0, Sux = 0.0, Svy = 0.0, Svx = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const int q = (k + 1) % NV;
        A2 = A2 + (dx[k] * dy[q] - dx[q] * dy[k]);
        const double us = u[q] + u[k], vs = v[q] + v[k], ddy = dy[q] - dy[k], ddx = dx[q] - dx[k];
        Suy = Suy + us * ddy; Sux = Sux + us * ddx;
        Svy = Svy + vs * ddy; Svx = Svx + vs * ddx;
    }
    ok = ok && A2 != 0.0 && finite64(A2);
    const double ux = Suy / A2, uy = -(Sux / A2), vx = Svy / A2, vy = -(Svx / A2);
    const double ar = 0.5 * fabs(A2);
    g[0] = ar;
    g[1] = ar * ux; g[2] = ar * uy; g[3] = ar * vx; g[4] = ar * vy;
    return ok;
}

// signed shoelace sum of DESIGN.md 3.9 on four points, relative to the first
__device__ __forceinline__ double shoelace4(const pt (&P)[4])
{
    double dx[4], dy[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { dx[k] = P[k].x - P[0].x; dy[k] = P[k].y - P[0].y; }
    double A2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = (k + 1) % 4;
        A2 = A2 + (dx[k] * dy[q] - dx[q] * dy[k]);
    }
    return A2;
}

// acceptance tests 1-4 and the score on a canonical quadrangle; +inf: not acceptable
__device__ __forceinline__ double quad_score(const pt (&P)[4], double A2, const QuadParams &c)
{
    double ex[4], ey[4], L[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int n = (k + 1) % 4;
        ex[k] = P[n].x - P[k].x; ey[k] = P[n].y - P[k].y;
        L[k] = ex[k] * ex[k] + ey[k] * ey[k];
    }
    bool ok = true;
    double score = 0.0, lmin = L[0], lmax = L[0];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int m = (k + 3) % 4;                                    // e_{k-1}
        const double cr = ex[m] * ey[k] - ey[m] * ex[k];
        ok = ok && cr > 0.0;
        const double ax = -ex[m], ay = -ey[m];
        const double d = ax * ex[k] + ay * ey[k];
        const double n = L[m] * L[k];
        const double s = d * fabs(d);
        ok = ok && s <= c.c_lo2 * n && s >= c.c_hi2 * n;
        const double qk = (d * d) / n;
        if (k == 0 || qk > score) score = qk;
        if (L[k] < lmin) lmin = L[k];
        if (L[k] > lmax) lmax = L[k];
    }
    ok = ok && lmin >= c.ratio2 * lmax;
    const double area = 0.5 * A2;
    ok = ok && c.area_min <= area && area <= c.area_max;
    ok = ok && score < plus_inf();                                    // a NaN or infinite score orders nothing
    return ok ? score : plus_inf();
}

}  // namespace sitrk
