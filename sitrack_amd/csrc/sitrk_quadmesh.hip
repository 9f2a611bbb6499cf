// sitrk_quadmesh.hip -- quadrangles from a triangulated buoy cloud (sitrk_tri2quad, sitrk_tri2quad_buoys): an EXTRA the reference does
// not have.  Adjacent triangles are paired into strictly convex, near-rectangular quadrangles by a deterministic greedy matching
// of maximum quality.  A translation unit of its own: no existing kernel is touched.  The contract (canonical form, acceptance
// tests, score, order of the matching) is in include/sitrk.h and DESIGN.md 3.12.
//
// Kernels, all one element per lane, memory bound, no LDS but the compaction's wave counts:
//   quad_mask_kernel     host arrays only: a point with mask 0 gets NaN in y, so "masked" and "not finite" are one test
//   quad_tri_kernel      one triangle per lane: index check (offenders counted by a vector atomic, never dereferenced), three
//                        16-byte gathers, the live/dead byte, and the triangle's three edge keys into the adjacency table
//   quad_score_kernel    one triangle per lane, three edges: neighbour and fourth point through the table, canonical form,
//                        acceptance tests, score (or +inf) and neighbour id (or -1) per triangle edge
//   quad_pick_kernel     a round, first half: every unmatched triangle picks its best edge whose neighbour is unmatched, by (score, key)
//   quad_match_kernel    a round, second half: mutual picks become pairs; one vector atomic per wave counts them
//   quad_count_kernel, quad_scan_kernel, quad_emit_kernel    the pairs in order of their smaller triangle id: flags counted per
//                        block, one workgroup scans the block counts, ballot + popcount ranks inside a block
//
// The adjacency table is open addressing on the 64-bit edge key (p << 32 | q, p < q) with linear probing, at least twice as many
// slots as half-edges; a slot is claimed with a 64-bit compare-and-swap, and next to the key one 64-bit word takes
// (t << 32) + 1 of every triangle t on the edge by atomic add: its low half is the number of triangles, its high half the sum
// of their ids modulo 2^32 -- for exactly two triangles, the other one is sum - t.  Sums do not depend on the order of arrival.
// Every probe loop is bounded by the number of slots; nothing waits for another lane.
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_cellmath.h"
#include "sitrk_internal.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kQmThreads = 256;
constexpr int kQmBlock = 1024;                      // elements per workgroup of the compaction
constexpr unsigned long long kQmEmpty = ~0ull;      // no edge key: p < q < 2^31

__device__ __forceinline__ uint64_t edge_slot(unsigned long long k, uint64_t mask)
{
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return k & mask;
}

__device__ __forceinline__ unsigned long long edge_key(int32_t a, int32_t b)
{
    const uint32_t p = (uint32_t)(a < b ? a : b), q = (uint32_t)(a < b ? b : a);
    return ((unsigned long long)p << 32) | q;
}

__global__ __launch_bounds__(kQmThreads) void quad_mask_kernel(int64_t n, const int8_t *__restrict__ mask, pt *__restrict__ p)
{
    const int64_t k = (int64_t)blockIdx.x * kQmThreads + threadIdx.x;
    if (k >= n) return;
    if (mask[k] == 0) p[k].y = quiet_nan();
}

// shoelace4() and quad_score() -- the signed area, the acceptance tests 1-4 and the score -- are in sitrk_cellmath.h

// The cycle r, p, s, q (p < q the shared edge, r != s the apexes) in canonical form: started at its smallest index, then
// counter-clockwise (A2 > 0).  false: A2 is 0, not finite or not positive after the turn.
__device__ __forceinline__ bool quad_canon(int32_t r, int32_t p, int32_t s, int32_t q, pt Pr, pt Pp, pt Ps, pt Pq, int32_t (&v)[4],
                                           pt (&P)[4], double &A2)
{
    const bool rs = r < s;
    const int32_t lo = rs ? r : s, hi = rs ? s : r;
    const pt Plo = rs ? Pr : Ps, Phi = rs ? Ps : Pr;
    const bool pf = p < lo;                                           // p first: p, lo, q, hi; else lo, p, hi, q
    v[0] = pf ? p : lo;   v[1] = pf ? lo : p;   v[2] = pf ? q : hi;   v[3] = pf ? hi : q;
    P[0] = pf ? Pp : Plo; P[1] = pf ? Plo : Pp; P[2] = pf ? Pq : Phi; P[3] = pf ? Phi : Pq;
    A2 = shoelace4(P);
    if (A2 < 0.0) {
        const int32_t tv = v[1]; v[1] = v[3]; v[3] = tv;
        const pt tp = P[1]; P[1] = P[3]; P[3] = tp;
        A2 = shoelace4(P);
    }
    return A2 > 0.0 && finite64(A2);
}

__global__ __launch_bounds__(kQmThreads) void quad_tri_kernel(int64_t nT, int64_t nP, const int32_t *__restrict__ tris,
                                                             const pt *__restrict__ pts, EdgeTable tab, int8_t *__restrict__ live,
                                                             unsigned long long *__restrict__ bad_index)
{
    const int64_t t = (int64_t)blockIdx.x * kQmThreads + threadIdx.x;
    if (t >= nT) return;
    int32_t v[3];
    bool in_range = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v[k] = tris[t * 3 + k];
        in_range = in_range && (uint64_t)(int64_t)v[k] < (uint64_t)nP;
    }
    if (!in_range) {
        atomicAdd(bad_index, 1ull);
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = 0;                         // point 0 stands in: the offending index is never dereferenced
    }
    pt P[3];
#pragma unroll
    for (int k = 0; k < 3; k++) P[k] = pts[v[k]];
    bool ok = in_range && v[0] != v[1] && v[1] != v[2] && v[2] != v[0];
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && finite64(P[k].y) && finite64(P[k].x);
    double dx[3], dy[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { dx[k] = P[k].x - P[0].x; dy[k] = P[k].y - P[0].y; }
    double A2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int q = (k + 1) % 3;
        A2 = A2 + (dx[k] * dy[q] - dx[q] * dy[k]);
    }
    ok = ok && A2 != 0.0 && finite64(A2);
    live[t] = ok ? 1 : 0;
    if (!ok) return;
    const unsigned long long add = ((unsigned long long)(uint32_t)t << 32) | 1ull;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned long long key = edge_key(v[k], v[(k + 1) % 3]);
        uint64_t slot = edge_slot(key, tab.mask);
        for (uint64_t i = 0; i <= tab.mask; i++) {                   // at most one look at every slot
            const unsigned long long old = atomicCAS(&tab.key[slot], kQmEmpty, key);
            if (old == kQmEmpty || old == key) {
                atomicAdd(&tab.val[slot], add);
                break;
            }
            slot = (slot + 1) & tab.mask;
        }
    }
}

__global__ __launch_bounds__(kQmThreads) void quad_score_kernel(int64_t nT, const int32_t *__restrict__ tris, const pt *__restrict__ pts,
                                                               EdgeTable tab, const int8_t *__restrict__ live, QuadParams c,
                                                               double *__restrict__ score, int32_t *__restrict__ nbr)
{
    const int64_t t = (int64_t)blockIdx.x * kQmThreads + threadIdx.x;
    if (t >= nT) return;
    double sc[3] = {plus_inf(), plus_inf(), plus_inf()};
    int32_t nb[3] = {-1, -1, -1};
    if (live[t]) {
        int32_t v[3];
        pt P[3];
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = tris[t * 3 + k];
#pragma unroll
        for (int k = 0; k < 3; k++) P[k] = pts[v[k]];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            const bool fwd = v[k] < v[k1];
            const int32_t p = fwd ? v[k] : v[k1], q = fwd ? v[k1] : v[k];
            const pt Pp = fwd ? P[k] : P[k1], Pq = fwd ? P[k1] : P[k];
            const unsigned long long key = edge_key(p, q);
            uint64_t slot = edge_slot(key, tab.mask);
            unsigned long long val = 0;
            for (uint64_t i = 0; i <= tab.mask; i++) {
                const unsigned long long kk = tab.key[slot];
                if (kk == key) { val = tab.val[slot]; break; }
                if (kk == kQmEmpty) break;
                slot = (slot + 1) & tab.mask;
            }
            if ((uint32_t)val != 2u) continue;                        // a border edge, or one of three and more triangles
            const uint32_t u = (uint32_t)(val >> 32) - (uint32_t)t;   // the other triangle: live, so its indices are in range
            if ((int64_t)u >= nT || (int64_t)u == t) continue;
            const int32_t w0 = tris[(int64_t)u * 3], w1 = tris[(int64_t)u * 3 + 1], w2 = tris[(int64_t)u * 3 + 2];
            const int32_t s = (w0 != p && w0 != q) ? w0 : (w1 != p && w1 != q) ? w1 : w2;
            if (s == v[k2] || s == p || s == q) continue;             // the same triangle listed twice
            const pt Ps = pts[s];
            int32_t cv[4];
            pt cp[4];
            double A2;
            if (!quad_canon(v[k2], p, s, q, P[k2], Pp, Ps, Pq, cv, cp, A2)) continue;
            const double qs = quad_score(cp, A2, c);
            sc[k] = qs;
            nb[k] = qs < plus_inf() ? (int32_t)u : -1;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        score[k * nT + t] = sc[k];
        nbr[k * nT + t] = nb[k];
    }
}

__global__ __launch_bounds__(kQmThreads) void quad_pick_kernel(int64_t nT, const int32_t *__restrict__ tris, const double *__restrict__ score,
                                                              const int32_t *__restrict__ nbr, const int32_t *__restrict__ mate,
                                                              int32_t *__restrict__ pick)
{
    const int64_t t = (int64_t)blockIdx.x * kQmThreads + threadIdx.x;
    if (t >= nT) return;
    int32_t best = -1;
    if (mate[t] < 0) {
        double bq = plus_inf();
        unsigned long long bkey = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int32_t u = nbr[k * nT + t];
            if (u < 0) continue;
            if (mate[u] >= 0) continue;
            const double qk = score[k * nT + t];
            const unsigned long long key = edge_key(tris[t * 3 + k], tris[t * 3 + (k + 1) % 3]);
            if (best < 0 || qk < bq || (qk == bq && key < bkey)) { best = u; bq = qk; bkey = key; }
        }
    }
    pick[t] = best;
}

__global__ __launch_bounds__(kQmThreads) void quad_match_kernel(int64_t nT, const int32_t *__restrict__ pick, int32_t *__restrict__ mate,
                                                               unsigned long long *__restrict__ matched)
{
    const int64_t t = (int64_t)blockIdx.x * kQmThreads + threadIdx.x;
    bool lead = false;
    if (t < nT) {
        const int32_t u = pick[t];
        if (u >= 0 && pick[u] == (int32_t)t) {
            mate[t] = u;
            lead = t < u;
        }
    }
    const unsigned long long bal = __ballot(lead);
    if (bal != 0ull && (threadIdx.x & 63) == 0) atomicAdd(matched, (unsigned long long)__popcll(bal));
}

// ---- the pairs in order of their smaller triangle id
__global__ __launch_bounds__(kQmBlock) void quad_count_kernel(int64_t nT, const int32_t *__restrict__ mate, unsigned *__restrict__ block_count)
{
    __shared__ unsigned sw[kQmBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kQmBlock + threadIdx.x;
    const bool f = t < nT && (int64_t)mate[t] > t;
    const unsigned long long bal = __ballot(f);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = (unsigned)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned n = 0;
        for (int w = 0; w < kQmBlock / 64; w++) n += sw[w];
        block_count[blockIdx.x] = n;
    }
}

// exclusive scan of the block counts by one workgroup (2^31 triangles -> 2^21 blocks: 2048 chunks at most)
__global__ __launch_bounds__(kQmBlock) void quad_scan_kernel(int64_t nblk, const unsigned *__restrict__ block_count,
                                                            int64_t *__restrict__ block_off, unsigned long long *__restrict__ total)
{
    __shared__ int64_t s_part[kQmBlock];
    __shared__ int64_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nblk; base += kQmBlock) {
        const int64_t k = base + threadIdx.x;
        const int64_t v = k < nblk ? (int64_t)block_count[k] : 0;
        s_part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kQmBlock; off <<= 1) {               // Hillis-Steele inclusive scan of this chunk
            const int64_t a = (int)threadIdx.x >= off ? s_part[threadIdx.x - off] : 0;
            __syncthreads();
            s_part[threadIdx.x] += a;
            __syncthreads();
        }
        const int64_t carry = s_carry;
        if (k < nblk) block_off[k] = carry + s_part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == kQmBlock - 1) s_carry = carry + s_part[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = (unsigned long long)s_carry;
}

__global__ __launch_bounds__(kQmBlock) void quad_emit_kernel(int64_t nT, int64_t cap, const int32_t *__restrict__ tris, const pt *__restrict__ pts,
                                                            const int8_t *__restrict__ live, const int32_t *__restrict__ mate,
                                                            const int64_t *__restrict__ block_off, int32_t *__restrict__ quads,
                                                            int32_t *__restrict__ tri_quad)
{
    __shared__ unsigned sw[kQmBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kQmBlock + threadIdx.x;
    const int32_t u = t < nT ? mate[t] : -1;
    const bool f = t < nT && (int64_t)u > t;
    const unsigned long long bal = __ballot(f);
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sw[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    if (t >= nT) return;
    if (u < 0) tri_quad[t] = live[t] ? -1 : -2;                       // a matched triangle's row is written by its pair's leader
    if (!f) return;
    unsigned rank = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    for (unsigned w = 0; w < wave; w++) rank += sw[w];
    const int64_t o = block_off[blockIdx.x] + rank;
    if (o >= cap) return;
    tri_quad[t] = (int32_t)o;
    tri_quad[u] = (int32_t)o;
    // the pair's quadrangle again, as quad_score_kernel formed it: shared edge = the two indices of t that u has too
    const int32_t a0 = tris[t * 3], a1 = tris[t * 3 + 1], a2 = tris[t * 3 + 2];
    const int32_t w0 = tris[(int64_t)u * 3], w1 = tris[(int64_t)u * 3 + 1], w2 = tris[(int64_t)u * 3 + 2];
    const bool in0 = a0 == w0 || a0 == w1 || a0 == w2, in1 = a1 == w0 || a1 == w1 || a1 == w2;
    const int32_t r = !in0 ? a0 : !in1 ? a1 : a2;
    const int32_t e0 = !in0 ? a1 : a0, e1 = (!in0 || !in1) ? a2 : a1;
    const int32_t p = e0 < e1 ? e0 : e1, q = e0 < e1 ? e1 : e0;
    const int32_t s = (w0 != p && w0 != q) ? w0 : (w1 != p && w1 != q) ? w1 : w2;
    int32_t cv[4];
    pt cp[4];
    double A2;
    (void)quad_canon(r, p, s, q, pts[r], pts[p], pts[s], pts[q], cv, cp, A2);
    int4 row;
    row.x = cv[0]; row.y = cv[1]; row.z = cv[2]; row.w = cv[3];
    ((int4 *)quads)[o] = row;
}

}  // namespace

}  // namespace sitrk

using namespace sitrk;

// the five parameters, checked before any device work (sitrk_mesh_build makes the same checks)
int sitrk::quad_check_params(sitrk_ctx *h, const char *fn, double cos_lo, double cos_hi, double ratio_min, double area_min, double area_max)
{
    if (!(cos_lo >= -1.0 && cos_lo <= 1.0 && cos_hi >= -1.0 && cos_hi <= 1.0 && cos_lo >= cos_hi))
        return fail(h, SITRK_EINVAL, "%s: need 1 >= cos_lo >= cos_hi >= -1 (got %g, %g)", fn, cos_lo, cos_hi);
    if (!(ratio_min >= 0.0 && ratio_min <= 1.0)) return fail(h, SITRK_EINVAL, "%s: ratio_min must be in [0,1] (got %g)", fn, ratio_min);
    if (!(area_min <= area_max)) return fail(h, SITRK_EINVAL, "%s: need area_min <= area_max (got %g, %g)", fn, area_min, area_max);
    return SITRK_OK;
}

static int quad_check(sitrk_ctx *h, const char *fn, int64_t nT, const int32_t *tris, double cos_lo, double cos_hi, double ratio_min,
                      double area_min, double area_max, int64_t cap, const int32_t *quads, const int32_t *tri_quad)
{
    if (!(nT >= 0 && nT < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nT must be in 0..2^31-2", fn);
    RCCHK(quad_check_params(h, fn, cos_lo, cos_hi, ratio_min, area_min, area_max));
    if (cap < nT / 2) return fail(h, SITRK_EINVAL, "%s: quads has room for %lld rows, %lld triangles need %lld", fn, (long long)cap,
                                  (long long)nT, (long long)(nT / 2));
    if (nT > 0 && !(tris && tri_quad && (quads || nT < 2))) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    return SITRK_OK;
}

static uint64_t quad_slots(int64_t nT)
{
    uint64_t s = 64;
    while (s < (uint64_t)6 * (uint64_t)nT) s <<= 1;                   // >= twice the 3 nT half-edges
    return s;
}

void sitrk::quad_carve(Carver &c, QuadBuffers &b, int64_t nT)
{
    b.slots = quad_slots(nT);
    b.tab.mask = b.slots - 1;
    c.take(b.tab.key, b.slots); c.take(b.tab.val, b.slots);
    c.take(b.tris, (size_t)3 * nT); c.take(b.live, nT);
    c.take(b.score, (size_t)3 * nT); c.take(b.nbr, (size_t)3 * nT);
    c.take(b.mate, nT); c.take(b.pick, nT);
    c.take(b.block_count, nblk(nT, kQmBlock)); c.take(b.block_off, nblk(nT, kQmBlock));
    c.take(b.quads, (size_t)4 * (nT / 2)); c.take(b.tri_quad, nT);
}

// The core: everything behind the points and the triangles, both on the device; the rows stay in b.quads / b.tri_quad.  The
// buffers may be carved for more triangles than nT: the adjacency table takes the slots of nT, which never changes a result.
int sitrk::quad_core(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_pts, int64_t nT, const int32_t *d_tris, const QuadBuffers &b,
                     const QuadParams &c, int64_t *nQ, int *rounds)
{
    RCCHK(h->quad_timer.begin(h));
    const uint64_t slots = quad_slots(nT);
    if (slots > b.slots) return fail(h, SITRK_EINVAL, "%s: %lld triangles do not fit the buffers", fn, (long long)nT);
    EdgeTable tab = b.tab;
    tab.mask = slots - 1;
    HIPCHK(hipMemsetAsync(h->counter, 0, 2 * sizeof(unsigned long long), h->stream));
    RCCHK(h->quad_timer.mark(h, 0));
    HIPCHK(hipMemsetAsync(tab.key, 0xff, slots * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(tab.val, 0, slots * sizeof(unsigned long long), h->stream));
    HIPCHK(hipMemsetAsync(b.mate, 0xff, (size_t)nT * sizeof(int32_t), h->stream));                  // -1: unmatched
    hipLaunchKernelGGL(quad_tri_kernel, dim3(nblk(nT, kQmThreads)), dim3(kQmThreads), 0, h->stream, nT, nP, d_tris, d_pts, tab, b.live, h->counter);
    HIPCHK(hipGetLastError());
    RCCHK(h->quad_timer.mark(h, 1));
    unsigned long long cnt[2] = {0, 0};
    HIPCHK(download(h, cnt, h->counter, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (cnt[0])                                                                                     // before any kernel follows an index
        return fail(h, SITRK_EINDEX, "%s: %llu triangle(s) have a vertex index outside [0, %lld)", fn, cnt[0], (long long)nP);
    hipLaunchKernelGGL(quad_score_kernel, dim3(nblk(nT, kQmThreads)), dim3(kQmThreads), 0, h->stream, nT, d_tris, d_pts, tab, b.live, c, b.score, b.nbr);
    HIPCHK(hipGetLastError());
    RCCHK(h->quad_timer.mark(h, 2));
    const int64_t max_rounds = nT / 2 + 1;
    int64_t nround = 0;
    unsigned long long before = 0;
    for (;;) {
        if (nround == max_rounds)
            return fail(h, SITRK_EINVAL, "%s: the matching has not come to rest after %lld rounds (%llu pairs)", fn, (long long)nround, before);
        hipLaunchKernelGGL(quad_pick_kernel, dim3(nblk(nT, kQmThreads)), dim3(kQmThreads), 0, h->stream, nT, d_tris, b.score, b.nbr, b.mate, b.pick);
        hipLaunchKernelGGL(quad_match_kernel, dim3(nblk(nT, kQmThreads)), dim3(kQmThreads), 0, h->stream, nT, b.pick, b.mate, h->counter + 1);
        HIPCHK(hipGetLastError());
        HIPCHK(download(h, cnt + 1, h->counter + 1, 1));
        HIPCHK(hipStreamSynchronize(h->stream));
        nround++;
        if (cnt[1] == before) break;
        before = cnt[1];
    }
    RCCHK(h->quad_timer.mark(h, 3));
    const int64_t nb = nblk(nT, kQmBlock);
    hipLaunchKernelGGL(quad_count_kernel, dim3((unsigned)nb), dim3(kQmBlock), 0, h->stream, nT, b.mate, b.block_count);
    hipLaunchKernelGGL(quad_scan_kernel, dim3(1), dim3(kQmBlock), 0, h->stream, nb, b.block_count, b.block_off, h->counter);
    hipLaunchKernelGGL(quad_emit_kernel, dim3((unsigned)nb), dim3(kQmBlock), 0, h->stream, nT, nT / 2, d_tris, d_pts, b.live, b.mate, b.block_off,
                       b.quads, b.tri_quad);
    HIPCHK(hipGetLastError());
    RCCHK(h->quad_timer.mark(h, 4));
    h->quad_timer.done();
    HIPCHK(download(h, cnt, h->counter, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (cnt[0] != cnt[1] || cnt[0] > (unsigned long long)(nT / 2))
        return fail(h, SITRK_EINVAL, "%s: %llu pairs matched, %llu compacted", fn, cnt[1], cnt[0]);
    *nQ = (int64_t)cnt[0];
    *rounds = (int)nround;
    return SITRK_OK;
}

// The host entry points: the triangles go up in front of the core, the rows come down behind it.
static int quad_run(sitrk_ctx *h, const char *fn, int64_t nP, const pt *d_pts, int64_t nT, const int32_t *tris, const QuadBuffers &b,
                    const QuadParams &c, int32_t *quads, int32_t *tri_quad, int64_t *nQ, int *rounds)
{
    HIPCHK(upload(h, b.tris, tris, (size_t)3 * nT));
    RCCHK(quad_core(h, fn, nP, d_pts, nT, b.tris, b, c, nQ, rounds));
    if (*nQ) HIPCHK(download(h, quads, b.quads, (size_t)4 * *nQ));
    HIPCHK(download(h, tri_quad, b.tri_quad, (size_t)nT));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

QuadParams sitrk::quad_params(double cos_lo, double cos_hi, double ratio_min, double area_min, double area_max)
{
    QuadParams c;
    c.c_lo2 = cos_lo * std::fabs(cos_lo);
    c.c_hi2 = cos_hi * std::fabs(cos_hi);
    c.ratio2 = ratio_min * ratio_min;
    c.area_min = area_min;
    c.area_max = area_max;
    return c;
}

SITRK_API int sitrk_tri2quad(sitrk_t *h, int64_t nP, const double *yx, const int8_t *mask, int64_t nT, const int32_t *tris, double cos_lo,
                             double cos_hi, double ratio_min, double area_min, double area_max, int64_t cap, int32_t *quads,
                             int32_t *tri_quad, int64_t *nQ, int *rounds)
{
    const char *fn = "sitrk_tri2quad";
    NEED(h, "null handle");
    RCCHK(quad_check(h, fn, nT, tris, cos_lo, cos_hi, ratio_min, area_min, area_max, cap, quads, tri_quad));
    if (!(nP >= 0 && nP < ((int64_t)1 << 31) - 1)) return fail(h, SITRK_EINVAL, "%s: nP must be in 0..2^31-2", fn);
    if (nP > 0 && !yx) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    int64_t nq = 0;
    int nr = 0;
    if (nQ) *nQ = 0;
    if (rounds) *rounds = 0;
    if (nT == 0) return SITRK_OK;
    if (nP == 0) return fail(h, SITRK_EINDEX, "%s: %lld triangle(s) have a vertex index outside [0, 0)", fn, (long long)nT);
    HIPCHK(hipSetDevice(h->device));
    pt *d_pts; int8_t *d_mask;
    QuadBuffers b;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_pts, nP); c.take(d_mask, nP); quad_carve(c, b, nT); }));
    HIPCHK(upload(h, d_pts, yx, nP));
    if (mask) {
        HIPCHK(upload(h, d_mask, mask, nP));
        hipLaunchKernelGGL(quad_mask_kernel, dim3(nblk(nP, kQmThreads)), dim3(kQmThreads), 0, h->stream, nP, d_mask, d_pts);
        HIPCHK(hipGetLastError());
    }
    RCCHK(quad_run(h, fn, nP, d_pts, nT, tris, b, quad_params(cos_lo, cos_hi, ratio_min, area_min, area_max), quads, tri_quad, &nq, &nr));
    if (nQ) *nQ = nq;
    if (rounds) *rounds = nr;
    return SITRK_OK;
}

SITRK_API int sitrk_tri2quad_buoys(sitrk_t *h, int64_t nT, const int32_t *tris, double cos_lo, double cos_hi, double ratio_min,
                                   double area_min, double area_max, int64_t cap, int32_t *quads, int32_t *tri_quad, int64_t *nQ,
                                   int *rounds)
{
    const char *fn = "sitrk_tri2quad_buoys";
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    RCCHK(quad_check(h, fn, nT, tris, cos_lo, cos_hi, ratio_min, area_min, area_max, cap, quads, tri_quad));
    int64_t nq = 0;
    int nr = 0;
    if (nQ) *nQ = 0;
    if (rounds) *rounds = 0;
    if (nT == 0) return SITRK_OK;
    HIPCHK(hipSetDevice(h->device));
    const int64_t nP = h->nP;
    pt *d_pts;
    QuadBuffers b;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_pts, nP); quad_carve(c, b, nT); }));
    RCCHK(deform_points_now(h, d_pts));
    RCCHK(quad_run(h, fn, nP, d_pts, nT, tris, b, quad_params(cos_lo, cos_hi, ratio_min, area_min, area_max), quads, tri_quad, &nq, &nr));
    if (nQ) *nQ = nq;
    if (rounds) *rounds = nr;
    return SITRK_OK;
}

SITRK_API int sitrk_tri2quad_kernel_ms(sitrk_t *h, float *adjacency_ms, float *score_ms, float *rounds_ms, float *compact_ms)
{
    NEED(h, "null handle");
    NEED(h->quad_timer.complete, "sitrk_tri2quad_kernel_ms: no tri2quad call has run all its kernels yet");
    float *out[4] = {adjacency_ms, score_ms, rounds_ms, compact_ms};
    for (int k = 0; k < 4; k++) RCCHK(h->quad_timer.elapsed(h, k, out[k]));
    return SITRK_OK;
}
