// sitrk_delaunay.hip -- bounded Delaunay triangulation of a buoy cloud (sitrk_delaunay, sitrk_delaunay_buoys): an EXTRA the reference
// does not have.  Every Delaunay triangle whose circumradius is at most rmax, decided by exact integer predicates on positions
// snapped to 2^-20 km.  A translation unit of its own: no existing kernel is touched.  The contract (vertices, predicates, size and
// reach tests, the tie rule, the order of the rows) is in include/sitrk.h and DESIGN.md 3.13.
//
// Kernels:
//   dl_quant_kernel    one point per lane: vertex or not, integer coordinates, bounding box / count / first coordinate out of range
//                      (reduced per workgroup, then one vector atomic each)
//   dl_key_kernel      cell key of every vertex (square cells of `side` units), ncells for everything else; rocPRIM's stable radix
//                      sort then orders the points by cell, index order inside a cell
//   dl_gather_kernel   coordinates in sorted order and cbeg[c] = first sorted slot of cell c (cells of one row are one run of slots)
//   dl_dup_kernel      a point with the coordinates of an earlier point of its cell is a duplicate: flag 2, coordinates "gone"
//   dl_tri_kernel      THE HOT KERNEL, one vertex p per lane.  For every q > p within reach: pass 1 over the neighbourhood finds the
//                      apex r left of p->q (replaced by s when s is strictly inside the circle p,q,r, or on it and right of
//                      q->r) and gives the pair up as soon as a vertex right of p->q lies strictly inside that circle; then the
//                      size and reach tests; pass 2 holds p,q,r against every vertex of the neighbourhood (conditions 4 and 5).  Rows go to a list through one vector atomic each.  No candidate list, no LDS, no scratch; every loop
//                      runs over a slot range read before it starts, nothing waits for another lane.
//   dl_rows_kernel     the rows in the order of their key p << 32 | q (one rocPRIM radix sort on the 64-bit keys) as (nT,3) int32
//
// In-circle: with u = q-p, v = r-p, w = s-p (|components| < 2^30, the reach box), A = ux*vy - uy*vx (int64),
// Bx = uy*|v|^2 - |u|^2*vy, By = ux*|v|^2 - |u|^2*vx (exact, __int128, once per apex), incircle(p,q,r,s) = -(wx*Bx - wy*By + |w|^2*A).
// The sign is first taken in fp64 with the error bound of DESIGN.md 3.13; only undecided lanes evaluate the __int128 form.
#include <cmath>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <stdint.h>

#include "sitrk_bins.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kDlThreads = 256;
constexpr int64_t kDlGone = (int64_t)1 << 62;      // coordinates of a point that is no vertex: outside every reach box
constexpr double kDlScale = 1048576.0;             // 2^20 units per km
constexpr double kDlMaxKm = 1073741824.0;          // 2^30 km

struct DlGrid {
    int64_t y0 = 0, x0 = 0, side = 1;   // cells of `side` units from (y0, x0)
    int64_t D = 0;                      // reach box: |dy|, |dx| <= D holds for every pair that passes the reach test
    int ny = 1, nx = 1, m = 1;          // m cells each way cover D
    uint32_t ncells = 1;
    double R4 = 0.0;                    // 4 * (ru * ru)
};

// red[0..3]: ymin, xmin, ymax, xmax of the vertices; red[4]: first index with a coordinate out of range; red[5]: vertices (with
// duplicates)
__global__ void dl_init_kernel(long long *red)
{
    if (threadIdx.x == 0) {
        red[0] = red[1] = 0x7fffffffffffffffll;
        red[2] = red[3] = -0x7fffffffffffffffll;
        red[4] = 0x7fffffffffffffffll;
        red[5] = 0;
    }
}

__global__ __launch_bounds__(kDlThreads) void dl_quant_kernel(int64_t n, const pt *__restrict__ p, const int8_t *__restrict__ mask,
                                                             ipt *__restrict__ xy, int8_t *__restrict__ vertex, long long *red)
{
    long long lo[2] = {0x7fffffffffffffffll, 0x7fffffffffffffffll}, hi[2] = {-0x7fffffffffffffffll, -0x7fffffffffffffffll};
    long long bad = 0x7fffffffffffffffll, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * kDlThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDlThreads) {
        const pt a = p[i];
        bool ok = (mask == nullptr || mask[i] != 0) && fabs(a.y) < INFINITY && fabs(a.x) < INFINITY;
        if (ok && (fabs(a.y) > kDlMaxKm || fabs(a.x) > kDlMaxKm)) {
            bad = min(bad, (long long)i);
            ok = false;
        }
        ipt q;
        q.y = q.x = kDlGone;
        if (ok) {
            q.y = __double2ll_rn(a.y * kDlScale);      // exact scaling, round to nearest even
            q.x = __double2ll_rn(a.x * kDlScale);
            lo[0] = min(lo[0], (long long)q.y); hi[0] = max(hi[0], (long long)q.y);
            lo[1] = min(lo[1], (long long)q.x); hi[1] = max(hi[1], (long long)q.x);
            cnt++;
        }
        xy[i] = q;
        vertex[i] = ok ? 1 : 0;
    }
    __shared__ long long sm[6][kDlThreads];
    sm[0][threadIdx.x] = lo[0]; sm[1][threadIdx.x] = lo[1];
    sm[2][threadIdx.x] = hi[0]; sm[3][threadIdx.x] = hi[1];
    sm[4][threadIdx.x] = bad;   sm[5][threadIdx.x] = cnt;
    __syncthreads();
    block_reduce<kDlThreads, Red::Min, Red::Min, Red::Max, Red::Max, Red::Min, Red::Add>(sm);
    if (threadIdx.x == 0) {
        if (sm[5][0]) {
            for (int c = 0; c < 2; c++) { atomicMin(&red[c], sm[c][0]); atomicMax(&red[2 + c], sm[2 + c][0]); }
            atomicAdd((unsigned long long *)&red[5], (unsigned long long)sm[5][0]);
        }
        if (sm[4][0] != 0x7fffffffffffffffll) atomicMin(&red[4], sm[4][0]);
    }
}

__global__ __launch_bounds__(kDlThreads) void dl_key_kernel(DlGrid g, int64_t n, const ipt *__restrict__ xy, uint32_t *__restrict__ key,
                                                           int32_t *__restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * kDlThreads + threadIdx.x;
    if (i >= n) return;
    const ipt a = xy[i];
    uint32_t k = g.ncells;
    if (a.y != kDlGone) {
        // deliberately not cell_coord of sitrk_bins.h: the coordinates are integers and the cell is their quotient by the side
        int64_t cy = (a.y - g.y0) / g.side, cx = (a.x - g.x0) / g.side;       // both differences are >= 0
        cy = cy < 0 ? 0 : (cy >= g.ny ? g.ny - 1 : cy);
        cx = cx < 0 ? 0 : (cx >= g.nx ? g.nx - 1 : cx);
        k = (uint32_t)(cy * g.nx + cx);
    }
    key[i] = k;
    val[i] = (int32_t)i;
}

// cbeg has ncells + 1 entries: the slots of cell c are [cbeg[c], cbeg[c+1]), everything behind cbeg[ncells] is no vertex.  Slot s
// writes the entries of the cells after its predecessor's up to its own: a loop over a count known when it starts.
__global__ __launch_bounds__(kDlThreads) void dl_gather_kernel(DlGrid g, int64_t n, const ipt *__restrict__ xy, const uint32_t *__restrict__ key,
                                                              const int32_t *__restrict__ perm, ipt *__restrict__ xys, int32_t *__restrict__ cbeg)
{
    const int64_t s = (int64_t)blockIdx.x * kDlThreads + threadIdx.x;
    if (s >= n) return;
    const int64_t k = key[s];
    const int64_t kp = s == 0 ? -1 : (int64_t)key[s - 1];
    xys[s] = xy[perm[s]];
    for (int64_t c = kp + 1; c <= k; c++) cbeg[c] = (int32_t)s;
    if (s == n - 1)
        for (int64_t c = k + 1; c <= (int64_t)g.ncells; c++) cbeg[c] = (int32_t)n;
}

__global__ __launch_bounds__(kDlThreads) void dl_dup_kernel(DlGrid g, int64_t nv, const ipt *__restrict__ xys, const uint32_t *__restrict__ key,
                                                           const int32_t *__restrict__ perm, const int32_t *__restrict__ cbeg,
                                                           ipt *__restrict__ out, int8_t *__restrict__ vertex)
{
    const int64_t s = (int64_t)blockIdx.x * kDlThreads + threadIdx.x;
    if (s >= nv) return;
    const ipt a = xys[s];
    bool dup = false;
    const int64_t b = cbeg[key[s]];
    for (int64_t t = b; t < s; t++) {                                         // lower indices of the same cell
        const ipt c = xys[t];
        dup = dup || (c.y == a.y && c.x == a.x);
    }
    ipt o = a;
    if (dup) {
        o.y = o.x = kDlGone;
        vertex[perm[s]] = 2;
    }
    out[s] = o;
}

// -------------------------------------------------------------------------------------------------- the hot kernel
struct Circle {                // the circle through p, q and the apex r, relative to p
    int32_t vx, vy;            // r - p
    int64_t A;                 // orient(p,q,r) > 0
    __int128 Bx, By;
    double Ad, Bxd, Byd;
};

__device__ __forceinline__ double i128_to_double(__int128 b)
{
    const bool neg = b < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)b : (unsigned __int128)b;
    const double d = (double)(uint64_t)(m >> 64) * 18446744073709551616.0 + (double)(uint64_t)m;   // both parts >= 0
    return neg ? -d : d;
}

__device__ __forceinline__ void circle_set(Circle &c, int32_t ux, int32_t uy, int64_t u2, int32_t vx, int32_t vy, int64_t A)
{
    const int64_t v2 = (int64_t)vx * vx + (int64_t)vy * vy;
    c.vx = vx; c.vy = vy; c.A = A;
    c.Bx = (__int128)uy * v2 - (__int128)u2 * vy;
    c.By = (__int128)ux * v2 - (__int128)u2 * vx;
    c.Ad = (double)A;
    c.Bxd = i128_to_double(c.Bx);
    c.Byd = i128_to_double(c.By);
}

// sign of incircle(p,q,r,s): +1 strictly inside, 0 on the circle, -1 outside
__device__ __forceinline__ int incircle_sign(const Circle &c, int32_t wx, int32_t wy, unsigned &nexact)
{
    const int64_t w2 = (int64_t)wx * wx + (int64_t)wy * wy;
    const double t1 = (double)wx * c.Bxd, t2 = (double)wy * c.Byd, t3 = (double)w2 * c.Ad;
    const double e = (t1 - t2) + t3;                                          // -incircle, rounded
    const double mag = (fabs(t1) + fabs(t2)) + fabs(t3);
    if (fabs(e) > 0x1p-49 * mag) return e < 0.0 ? 1 : -1;
    nexact++;
    const __int128 x = (__int128)wx * c.Bx - (__int128)wy * c.By + (__int128)w2 * c.A;
    return x < 0 ? 1 : (x > 0 ? -1 : 0);
}

// orient(q,r,s) from the differences to p
__device__ __forceinline__ int64_t orient_qrs(int32_t ux, int32_t uy, int32_t vx, int32_t vy, int32_t wx, int32_t wy)
{
    return ((int64_t)vx - ux) * ((int64_t)wy - uy) - ((int64_t)vy - uy) * ((int64_t)wx - ux);
}

__device__ __forceinline__ bool in_box(int64_t d, int64_t D) { return (uint64_t)(d + D) <= (uint64_t)(2 * D); }

__global__ __launch_bounds__(kDlThreads) void dl_tri_kernel(DlGrid g, int64_t nv, const ipt *__restrict__ xy, const uint32_t *__restrict__ key,
                                                           const int32_t *__restrict__ perm, const int32_t *__restrict__ cbeg,
                                                           int64_t cap_rows, unsigned long long *__restrict__ rkey, int32_t *__restrict__ rval,
                                                           unsigned long long *__restrict__ counter)
{
    const int64_t s0 = (int64_t)blockIdx.x * kDlThreads + threadIdx.x;
    unsigned long long ntest = 0;
    unsigned nexact = 0;
    ipt P;
    P.y = P.x = kDlGone;
    if (s0 < nv) P = xy[s0];
    if (P.y != kDlGone) {
        const int32_t pi = perm[s0];
        const uint32_t k = key[s0];
        const int cy = (int)(k / (uint32_t)g.nx), cx = (int)(k % (uint32_t)g.nx);
        const int xa = max(cx - g.m, 0), xb = min(cx + g.m, g.nx - 1);
        const int nrow = 2 * g.m + 1;                                          // rows cy, cy-1, cy+1, ...: the nearest first
        for (int jq = 0; jq < nrow; jq++) {
            const int qy = (jq & 1) ? cy - ((jq + 1) >> 1) : cy + ((jq + 1) >> 1);
            if (qy < 0 || qy >= g.ny) continue;
            const int32_t qe = cbeg[(int64_t)qy * g.nx + xb + 1];
            for (int32_t qs = cbeg[(int64_t)qy * g.nx + xa]; qs < qe; qs++) {
                const int32_t qi = perm[qs];
                if (qi <= pi) continue;
                const ipt Q = xy[qs];
                const int64_t duy = Q.y - P.y, dux = Q.x - P.x;
                if (!in_box(duy, g.D) || !in_box(dux, g.D)) continue;
                const int32_t ux = (int32_t)dux, uy = (int32_t)duy;
                const int64_t u2 = (int64_t)ux * ux + (int64_t)uy * uy;
                const double la = (double)u2;
                if (!(la <= g.R4)) continue;
                // pass 1: the apex among ALL vertices left of p->q (c, slot rs) and the vertex right of it whose circle through p
                // and q reaches furthest to the left (cb).  A valid triangle has the first as its r: a lower-indexed apex lies in
                // or on the circle of any other.  As soon as the vertex on the right is strictly inside the circle of the one on
                // the left, no empty circle passes through p and q and the pair is done.
                int32_t rs = -1;
                bool right = false, dead = false;
                Circle c, cb;
                c.vx = c.vy = 0; c.A = 0; c.Bx = c.By = 0; c.Ad = c.Bxd = c.Byd = 0.0;
                cb = c;
                for (int js = 0; js < nrow && !dead; js++) {
                    const int sy = (js & 1) ? cy - ((js + 1) >> 1) : cy + ((js + 1) >> 1);
                    if (sy < 0 || sy >= g.ny) continue;
                    const int32_t se = cbeg[(int64_t)sy * g.nx + xb + 1];
                    for (int32_t ss = cbeg[(int64_t)sy * g.nx + xa]; ss < se && !dead; ss++) {
                        const ipt S = xy[ss];
                        const int64_t dwy = S.y - P.y, dwx = S.x - P.x;
                        if (!in_box(dwy, g.D) || !in_box(dwx, g.D)) continue;
                        const int32_t wx = (int32_t)dwx, wy = (int32_t)dwy;
                        const int64_t o = (int64_t)ux * wy - (int64_t)uy * wx;       // orient(p,q,s): 0 for s = p and s = q
                        if (o == 0) continue;
                        bool take;
                        if (o > 0) {
                            take = rs < 0;
                            if (!take) {
                                ntest++;
                                const int sg = incircle_sign(c, wx, wy, nexact);
                                take = sg > 0 || (sg == 0 && orient_qrs(ux, uy, c.vx, c.vy, wx, wy) < 0);
                            }
                            if (take) {
                                rs = ss;
                                circle_set(c, ux, uy, u2, wx, wy, o);
                            }
                        } else {
                            take = !right;
                            if (!take) {
                                ntest++;
                                take = incircle_sign(cb, wx, wy, nexact) < 0;           // p,q,b is clockwise: the sign is turned
                            }
                            if (take) {
                                right = true;
                                circle_set(cb, ux, uy, u2, wx, wy, o);
                            }
                        }
                        if (take && right && rs >= 0) {
                            ntest++;
                            dead = incircle_sign(c, cb.vx, cb.vy, nexact) > 0;
                        }
                    }
                }
                if (dead || rs < 0) continue;
                if (perm[rs] <= pi) continue;
                // conditions 2 and 3
                const int64_t ex = (int64_t)c.vx - ux, ey = (int64_t)c.vy - uy;
                const double lb = (double)((int64_t)c.vx * c.vx + (int64_t)c.vy * c.vy);
                const double lc = (double)(ex * ex + ey * ey);
                if (!(lb <= g.R4 && lc <= g.R4)) continue;
                const double lhs = (la * lb) * lc, rhs = (g.R4 * c.Ad) * c.Ad;
                if (!(lhs <= rhs)) continue;
                // pass 2: conditions 4 and 5 against every vertex of the neighbourhood
                bool ok = true;
                for (int js = 0; js < nrow && ok; js++) {
                    const int sy = (js & 1) ? cy - ((js + 1) >> 1) : cy + ((js + 1) >> 1);
                    if (sy < 0 || sy >= g.ny) continue;
                    const int32_t se = cbeg[(int64_t)sy * g.nx + xb + 1];
                    for (int32_t ss = cbeg[(int64_t)sy * g.nx + xa]; ss < se && ok; ss++) {
                        if (ss == (int32_t)s0 || ss == qs || ss == rs) continue;
                        const ipt S = xy[ss];
                        const int64_t dwy = S.y - P.y, dwx = S.x - P.x;
                        if (!in_box(dwy, g.D) || !in_box(dwx, g.D)) continue;
                        const int32_t wx = (int32_t)dwx, wy = (int32_t)dwy;
                        ntest++;
                        const int sg = incircle_sign(c, wx, wy, nexact);
                        if (sg > 0) ok = false;
                        else if (sg == 0) ok = perm[ss] > pi && orient_qrs(ux, uy, c.vx, c.vy, wx, wy) > 0;
                    }
                }
                if (!ok) continue;
                const unsigned long long o = atomicAdd(&counter[0], 1ull);
                if ((int64_t)o < cap_rows) {
                    rkey[o] = ((unsigned long long)(uint32_t)pi << 32) | (uint32_t)qi;
                    rval[o] = perm[rs];
                }
            }
        }
    }
    unsigned long long nex = nexact;                                          // every lane of the wave is here: one sum per wave
    for (int o = 32; o > 0; o >>= 1) {
        ntest += __shfl_xor(ntest, o);
        nex += __shfl_xor(nex, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (ntest) atomicAdd(&counter[1], ntest);
        if (nex) atomicAdd(&counter[2], nex);
    }
}

__global__ __launch_bounds__(kDlThreads) void dl_rows_kernel(int64_t nT, const unsigned long long *__restrict__ rkey, const int32_t *__restrict__ rval,
                                                            int32_t *__restrict__ tris)
{
    const int64_t t = (int64_t)blockIdx.x * kDlThreads + threadIdx.x;
    if (t >= nT) return;
    const unsigned long long k = rkey[t];
    tris[3 * t] = (int32_t)(k >> 32);
    tris[3 * t + 1] = (int32_t)(k & 0xffffffffull);
    tris[3 * t + 2] = rval[t];
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kDlThreads - 1) / kDlThreads); }

hipError_t sort_rows_u64(void *tmp, size_t *tmp_bytes, const unsigned long long *kin, unsigned long long *kout, const int32_t *vin,
                         int32_t *vout, size_t n, unsigned end_bit, hipStream_t s)
{
    return rocprim::radix_sort_pairs(tmp, *tmp_bytes, kin, kout, vin, vout, n, 0u, end_bit, s);
}

}  // namespace

}  // namespace sitrk

using namespace sitrk;

int sitrk::dl_check_rmax(sitrk_ctx *h, const char *fn, double rmax_km)
{
    if (!std::isfinite(rmax_km) || !(rmax_km > 0.0) || rmax_km > 500.0)
        return fail(h, SITRK_EINVAL, "%s: rmax_km must be finite and in (0, 500] (got %g)", fn, rmax_km);
    return SITRK_OK;
}

static int dl_check(sitrk_ctx *h, const char *fn, double rmax_km, int64_t cap, const int32_t *tris, const int64_t *nT)
{
    RCCHK(dl_check_rmax(h, fn, rmax_km));
    if (!nT) return fail(h, SITRK_EINVAL, "%s: null nT", fn);
    if (cap < 0) return fail(h, SITRK_EINVAL, "%s: cap must be >= 0", fn);
    if (cap > 0 && !tris) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    return SITRK_OK;
}

// The layout of the scratch behind d_pts / d_mask is carved by the caller through dl_carve.
int sitrk::dl_sort_bytes(sitrk_ctx *h, int64_t nP, size_t *bytes)
{
    size_t b32 = 0, b64 = 0;
    HIPCHK(sort_pairs_u32(nullptr, &b32, nullptr, nullptr, nullptr, nullptr, (size_t)nP, 32, h->stream));
    HIPCHK(sort_rows_u64(nullptr, &b64, nullptr, nullptr, nullptr, nullptr, (size_t)2 * nP, 64, h->stream));
    *bytes = align256(b32 > b64 ? b32 : b64);
    return SITRK_OK;
}

void sitrk::dl_carve(Carver &c, DlBuffers &b, int64_t nP)
{
    const size_t n = (size_t)nP, rows = 2 * n;           // nT <= 2 nV - 5
    c.take(b.xy, n); c.take(b.xys, n); c.take(b.xyv, n);
    c.take(b.k0, n); c.take(b.k1, n); c.take(b.v0, n); c.take(b.perm, n);
    c.take(b.cbeg, n + 1024 + 1);
    c.take(b.vertex, n);
    c.take(b.rkey0, rows); c.take(b.rkey1, rows); c.take(b.rval0, rows); c.take(b.rval1, rows);
    c.take(b.tris, 3 * rows);
    c.take(b.red, 8);
    c.take(b.sort_tmp, b.sort_bytes);
}

// The core: everything behind the points.  d_pts (nP; masked by d_mask when given) is on the device and the stream is behind what
// made it; the rows stay in b.tris, the vertex bytes in b.vertex.
int sitrk::dl_core(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_pts, const int8_t *d_mask, const DlBuffers &b, double rmax_km,
                   int64_t *nT)
{
    const hipStream_t st = h->stream;                    // the stream the timer marks
    RCCHK(h->dl_timer.begin(h));
    HIPCHK(hipMemsetAsync(h->counter, 0, 4 * sizeof(unsigned long long), st));
    RCCHK(h->dl_timer.mark(h, 0));
    hipLaunchKernelGGL(dl_init_kernel, dim3(1), dim3(64), 0, st, b.red);
    hipLaunchKernelGGL(dl_quant_kernel, dim3(nblk(nP) < 2048u ? nblk(nP) : 2048u), dim3(kDlThreads), 0, st, nP, d_pts, d_mask, b.xy, b.vertex, b.red);
    HIPCHK(hipGetLastError());
    long long red[6];
    HIPCHK(download(h, red, b.red, 6));
    HIPCHK(hipStreamSynchronize(st));
    if (red[4] != 0x7fffffffffffffffll)
        return fail(h, SITRK_EINVAL, "%s: coordinate beyond 2^30 km at index %lld", fn, red[4]);
    const int64_t nv = red[5];
    unsigned long long cnt[3] = {0, 0, 0};
    if (nv > 0) {
        DlGrid g;
        const double ru = rmax_km * kDlScale;
        g.R4 = 4.0 * (ru * ru);
        g.D = (int64_t)std::floor(2.0 * ru) + 2;        // la <= R4 in fp64 leaves |d| <= 2 ru (1 + 2^-52) < floor(2 ru) + 2
        g.m = h->delaunay_bin;
        g.side = (g.D + g.m - 1) / g.m;                  // m cells cover D
        g.y0 = red[0]; g.x0 = red[1];
        const int64_t max_cells = nP + 1024;
        int64_t ny, nx;
        for (;;) {                                       // a coarser grid is only slower
            ny = (red[2] - red[0]) / g.side + 1;
            nx = (red[3] - red[1]) / g.side + 1;
            if (ny <= (1 << 20) && nx <= (1 << 20) && ny * nx <= max_cells) break;
            g.side *= 2;
        }
        g.ny = (int)ny; g.nx = (int)nx;
        g.ncells = (uint32_t)(ny * nx);
        const unsigned end_bit = key_bits(g.ncells);     // keys 0..ncells (ncells: no vertex)
        hipLaunchKernelGGL(dl_key_kernel, dim3(nblk(nP)), dim3(kDlThreads), 0, st, g, nP, b.xy, b.k0, b.v0);
        HIPCHK(hipGetLastError());
        size_t tb = b.sort_bytes;
        HIPCHK(sort_pairs_u32(b.sort_tmp, &tb, b.k0, b.k1, b.v0, b.perm, (size_t)nP, end_bit, st));
        hipLaunchKernelGGL(dl_gather_kernel, dim3(nblk(nP)), dim3(kDlThreads), 0, st, g, nP, b.xy, b.k1, b.perm, b.xys, b.cbeg);
        hipLaunchKernelGGL(dl_dup_kernel, dim3(nblk(nv)), dim3(kDlThreads), 0, st, g, nv, b.xys, b.k1, b.perm, b.cbeg, b.xyv, b.vertex);
        HIPCHK(hipGetLastError());
        RCCHK(h->dl_timer.mark(h, 1));
        const int64_t cap_rows = 2 * nP;
        hipLaunchKernelGGL(dl_tri_kernel, dim3(nblk(nv)), dim3(kDlThreads), 0, st, g, nv, b.xyv, b.k1, b.perm, b.cbeg, cap_rows, b.rkey0,
                           b.rval0, h->counter);
        HIPCHK(hipGetLastError());
        RCCHK(h->dl_timer.mark(h, 2));
        HIPCHK(download(h, cnt, h->counter, 3));
        HIPCHK(hipStreamSynchronize(st));
        if (cnt[0] > (unsigned long long)cap_rows)
            return fail(h, SITRK_EHIP, "%s: %llu triangles on %lld vertices", fn, cnt[0], (long long)nv);
        if (cnt[0]) {
            const unsigned pbits = key_bits((uint64_t)nP - 1);    // p and q are indices below nP
            tb = b.sort_bytes;
            HIPCHK(sort_rows_u64(b.sort_tmp, &tb, b.rkey0, b.rkey1, b.rval0, b.rval1, (size_t)cnt[0], 32 + pbits, st));
            hipLaunchKernelGGL(dl_rows_kernel, dim3(nblk((int64_t)cnt[0])), dim3(kDlThreads), 0, st, (int64_t)cnt[0], b.rkey1, b.rval1, b.tris);
            HIPCHK(hipGetLastError());
        }
        RCCHK(h->dl_timer.mark(h, 3));
        h->dl_timer.done();
    }
    h->dl_tests = cnt[1];
    h->dl_exact = cnt[2];
    *nT = (int64_t)cnt[0];
    return SITRK_OK;
}

// The host entry points: the rows and the vertex bytes come down behind the core.
static int dl_run(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_pts, const int8_t *d_mask, const DlBuffers &b, double rmax_km,
                  int64_t cap, int32_t *tris, int64_t *nT, int8_t *vertex)
{
    RCCHK(dl_core(h, fn, nP, d_pts, d_mask, b, rmax_km, nT));
    if (*nT && cap >= *nT) HIPCHK(download(h, tris, b.tris, (size_t)3 * *nT));
    if (vertex) HIPCHK(download(h, vertex, b.vertex, (size_t)nP));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

SITRK_API int sitrk_delaunay(sitrk_t *h, int64_t nP, const double *yx, const int8_t *mask, double rmax_km, int64_t cap, int32_t *tris,
                             int64_t *nT, int8_t *vertex)
{
    const char *fn = "sitrk_delaunay";
    NEED(h, "null handle");
    RCCHK(dl_check(h, fn, rmax_km, cap, tris, nT));
    if (!(nP >= 0 && nP < ((int64_t)1 << 30))) return fail(h, SITRK_EINVAL, "%s: nP must be in 0..2^30-1", fn);
    if (nP > 0 && !yx) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    *nT = 0;
    if (nP == 0) return SITRK_OK;
    HIPCHK(hipSetDevice(h->device));
    pt *d_pts; int8_t *d_mask;
    DlBuffers b;
    RCCHK(dl_sort_bytes(h, nP, &b.sort_bytes));
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_pts, nP); c.take(d_mask, nP); dl_carve(c, b, nP); }));
    HIPCHK(upload(h, d_pts, yx, nP));
    if (mask) HIPCHK(upload(h, d_mask, mask, nP));
    return dl_run(h, fn, nP, d_pts, mask ? d_mask : nullptr, b, rmax_km, cap, tris, nT, vertex);
}

SITRK_API int sitrk_delaunay_buoys(sitrk_t *h, double rmax_km, int64_t cap, int32_t *tris, int64_t *nT, int8_t *vertex)
{
    const char *fn = "sitrk_delaunay_buoys";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    RCCHK(dl_check(h, fn, rmax_km, cap, tris, nT));
    const int64_t nP = h->nP;
    if (!(nP < ((int64_t)1 << 30))) return fail(h, SITRK_EINVAL, "%s: more than 2^30-1 buoys", fn);
    *nT = 0;
    HIPCHK(hipSetDevice(h->device));
    pt *d_pts;
    DlBuffers b;
    RCCHK(dl_sort_bytes(h, nP, &b.sort_bytes));
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_pts, nP); dl_carve(c, b, nP); }));
    RCCHK(deform_points_now(h, d_pts));              // NaN in y: not alive now, no vertex
    return dl_run(h, fn, nP, d_pts, nullptr, b, rmax_km, cap, tris, nT, vertex);
}

SITRK_API int sitrk_delaunay_kernel_ms(sitrk_t *h, float *bin_ms, float *tri_ms, float *compact_ms)
{
    NEED(h, "null handle");
    NEED(h->dl_timer.complete, "sitrk_delaunay_kernel_ms: no delaunay call has run all its kernels yet");
    float *out[3] = {bin_ms, tri_ms, compact_ms};
    for (int k = 0; k < 3; k++) RCCHK(h->dl_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}

SITRK_API int sitrk_delaunay_stats(sitrk_t *h, int64_t *incircle_tests, int64_t *exact_tests)
{
    NEED(h, "null handle");
    if (incircle_tests) *incircle_tests = (int64_t)h->dl_tests;
    if (exact_tests) *exact_tests = (int64_t)h->dl_exact;
    return SITRK_OK;
}
