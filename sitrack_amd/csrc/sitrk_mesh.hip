// sitrk_mesh.hip -- device-resident quadrangle meshes (sitrk_mesh_*): an EXTRA the reference does not have.  The chain bounded
// Delaunay triangulation -> pairing into quadrangles -> deformation rates with nothing but counters crossing to the host: the
// cores of sitrk_delaunay.hip and sitrk_quadmesh.hip run back to back out of one scratch layout, the quadrangles and the t0
// positions of their vertices stay in allocations of the mesh's own, and every analysis time is one pass over the buoys, one
// cell kernel and one final sum.  The contract is in include/sitrk.h and DESIGN.md 3.14; the per-cell arithmetic is that of
// sitrk_cellmath.h, shared with deform_cells_kernel<4> and quad_score_kernel.
//
// Kernels, wave64, 256 lanes per workgroup, memory bound, no scratch memory, LDS only for the reduction (320 B):
//   mesh_mask_kernel    one buoy per lane: NaN in y where the mask byte is 0, so "masked" and "not alive" are one test
//   mesh_t0_kernel      one quadrangle per lane: its four indices (one dwordx4), four 16-byte gathers, 64 B written in cell order
//   mesh_cells_kernel   one quadrangle per lane: its indices, its contiguous t0 block and four t1 gathers, the rates of DESIGN.md
//                       3.9, the acceptance of 3.12 at t1, stores behind wave-uniform tests on the output pointers, and ten partial
//                       terms per lane summed over the wave (xor butterfly) and the workgroup (waves 0..3 in order) into one row of
//                       a (blocks,10) array
//   mesh_sum_kernel     one workgroup: lane l sums the rows l, l+256, ... in order, then the same wave and workgroup reduction
// Every loop is bounded by a count read before it starts, no lane waits for another, no floating-point atomics: the order of
// every sum is fixed by the launch geometry alone.
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_cellmath.h"
#include "sitrk_internal.h"
#include "sitrk_reduce.h"

#pragma clang fp contract(off)

namespace sitrk {

namespace {

constexpr int kMeshThreads = 256;
constexpr int kMeshStats = SITRK_MESH_NSTATS;

__global__ __launch_bounds__(kMeshThreads) void mesh_mask_kernel(int64_t n, const int8_t *__restrict__ mask, pt *__restrict__ p)
{
    const int64_t k = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (k >= n) return;
    if (mask[k] == 0) p[k].y = quiet_nan();
}

__global__ __launch_bounds__(kMeshThreads) void mesh_t0_kernel(int64_t nQ, const int4 *__restrict__ quads, const pt *__restrict__ pts,
                                                              pt *__restrict__ t0)
{
    const int64_t c = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (c >= nQ) return;
    const int4 q = quads[c];
    const pt a0 = pts[q.x], a1 = pts[q.y], a2 = pts[q.z], a3 = pts[q.w];
    t0[4 * c] = a0; t0[4 * c + 1] = a1; t0[4 * c + 2] = a2; t0[4 * c + 3] = a3;
}

__global__ __launch_bounds__(kMeshThreads) void mesh_cells_kernel(int64_t nQ, const int4 *__restrict__ quads, const pt *__restrict__ t0,
                                                                 const pt *__restrict__ p1, double T, QuadParams par,
                                                                 double *__restrict__ out, int8_t *__restrict__ status,
                                                                 double *__restrict__ partials)
{
    __shared__ double sm[kMeshThreads / 64][kMeshStats];
    const int64_t c0 = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    const bool live = c0 < nQ;                                         // a lane behind the last cell reads the last cell and adds zeros
    const int64_t c = live ? c0 : nQ - 1;
    const int4 q = quads[c];
    pt a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = t0[4 * c + k];
    b[0] = p1[q.x]; b[1] = p1[q.y]; b[2] = p1[q.z]; b[3] = p1[q.w];

    double r[5];
    const bool ok = deform_rates<4>(a, b, T, r);
    const double B2 = shoelace4(b);                                    // DESIGN.md 3.12 on the stored order at t1
    const bool acc = B2 > 0.0 && finite64(B2) && quad_score(b, B2, par) < plus_inf();
    const int st = !ok ? 0 : (acc ? 1 : 2);

    if (out != nullptr && live) {
        const double fill = SITRK_FILL;
#pragma unroll
        for (int k = 0; k < 5; k++) out[k * nQ + c] = ok ? r[k] : fill;
    }
    if (status != nullptr && live) status[c] = (int8_t)st;
    if (partials == nullptr) return;                                   // wave-uniform, as the two tests above

    const bool s1 = live && st == 1;
    const double ar = r[3];
    const double tot = sqrt(r[0] * r[0] + r[1] * r[1]);
    const double m1 = ar * tot, m2 = m1 * tot, m3 = m2 * tot;
    double t[kMeshStats];
    t[0] = live && st == 0 ? 1.0 : 0.0;
    t[1] = s1 ? 1.0 : 0.0;
    t[2] = live && st == 2 ? 1.0 : 0.0;
    t[3] = s1 ? ar : 0.0;
    t[4] = s1 ? r[4] : 0.0;
    t[5] = s1 ? ar * r[0] : 0.0;
    t[6] = s1 ? ar * r[1] : 0.0;
    t[7] = s1 ? m1 : 0.0;
    t[8] = s1 ? m2 : 0.0;
    t[9] = s1 ? m3 : 0.0;
    const double s = block_sum<kMeshStats, kMeshThreads>(t, sm);
    if (threadIdx.x < kMeshStats) partials[(int64_t)blockIdx.x * kMeshStats + threadIdx.x] = s;
}

__global__ __launch_bounds__(kMeshThreads) void mesh_sum_kernel(int64_t nrows, const double *__restrict__ partials, double *__restrict__ stats)
{
    __shared__ double sm[kMeshThreads / 64][kMeshStats];
    double t[kMeshStats];
#pragma unroll
    for (int k = 0; k < kMeshStats; k++) t[k] = 0.0;
    for (int64_t row = threadIdx.x; row < nrows; row += kMeshThreads) {
#pragma unroll
        for (int k = 0; k < kMeshStats; k++) t[k] = t[k] + partials[row * kMeshStats + k];
    }
    const double s = block_sum<kMeshStats, kMeshThreads>(t, sm);
    if (threadIdx.x < kMeshStats) stats[threadIdx.x] = s;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kMeshThreads - 1) / kMeshThreads); }

void mesh_free_one(Mesh &m)
{
    if (m.quads) (void)hipFree(m.quads);
    if (m.t0) (void)hipFree(m.t0);
    m = Mesh();
}

}  // namespace

void mesh_release(sitrk_ctx *h, bool destroy)
{
    for (Mesh &m : h->mesh) mesh_free_one(m);
    h->mesh_deform_timer.complete = false;
    if (destroy) {
        h->mesh_build_timer.release();
        h->mesh_deform_timer.release();
    }
}

}  // namespace sitrk

using namespace sitrk;

// what every entry point checks first: the handle's buoys and the slot number
static int mesh_check(sitrk_ctx *h, const char *fn, int mesh, bool need_built)
{
    if (mesh < 0 || mesh >= SITRK_MESH_MAX) return fail(h, SITRK_EINVAL, "%s: mesh must be in 0..%d (got %d)", fn, SITRK_MESH_MAX - 1, mesh);
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    if (need_built && !h->mesh[mesh].built)
        return fail(h, SITRK_EINVAL, "%s: mesh %d is empty (call sitrk_mesh_build first; sitrk_set_buoys frees every mesh)", fn, mesh);
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_build(sitrk_t *h, int mesh, int jrec0, double rmax_km, const int8_t *mask, double cos_lo, double cos_hi,
                               double ratio_min, double area_min, double area_max, int64_t *nT, int64_t *nQ, int *rounds)
{
    const char *fn = "sitrk_mesh_build";
    NEED(h, "null handle");
    RCCHK(mesh_check(h, fn, mesh, false));
    RCCHK(dl_check_rmax(h, fn, rmax_km));
    RCCHK(quad_check_params(h, fn, cos_lo, cos_hi, ratio_min, area_min, area_max));
    const int64_t nP = h->nP;
    if (!(nP < ((int64_t)1 << 30))) return fail(h, SITRK_EINVAL, "%s: more than 2^30-1 buoys", fn);
    if (nT) *nT = 0;
    if (nQ) *nQ = 0;
    if (rounds) *rounds = 0;
    HIPCHK(hipSetDevice(h->device));
    RCCHK(h->mesh_build_timer.begin(h));
    const QuadParams par = quad_params(cos_lo, cos_hi, ratio_min, area_min, area_max);
    // one layout for the whole chain: the points, the mask, the buffers of both cores (nT <= 2 nP - 5 triangles)
    pt *d_pts; int8_t *d_mask;
    DlBuffers db;
    QuadBuffers qb;
    RCCHK(dl_sort_bytes(h, nP, &db.sort_bytes));
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_pts, nP); c.take(d_mask, nP); dl_carve(c, db, nP); quad_carve(c, qb, 2 * nP); }));
    if (mask) HIPCHK(upload(h, d_mask, mask, nP));
    RCCHK(h->mesh_build_timer.mark(h, 0));
    RCCHK(deform_points_now(h, d_pts));                  // NaN in y: not alive now
    if (mask) {
        hipLaunchKernelGGL(mesh_mask_kernel, dim3(nblk(nP)), dim3(kMeshThreads), 0, h->stream, nP, d_mask, d_pts);
        HIPCHK(hipGetLastError());
    }
    int64_t nt = 0, nq = 0;
    int nr = 0;
    RCCHK(dl_core(h, fn, nP, d_pts, nullptr, db, rmax_km, &nt));
    if (nt > 0) RCCHK(quad_core(h, fn, nP, d_pts, nt, db.tris, qb, par, &nq, &nr));
    Mesh m;
    m.built = true;
    m.nQ = nq;
    m.jrec0 = jrec0;
    m.rmax_km = rmax_km;
    m.par = par;
    if (nq > 0) {
        if (hipMalloc((void **)&m.quads, (size_t)nq * 4 * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void **)&m.t0, (size_t)nq * 4 * sizeof(pt)) != hipSuccess) {
            mesh_free_one(m);
            return fail(h, SITRK_EHIP, "%s: no device memory for %lld quadrangles", fn, (long long)nq);
        }
        hipError_t e = hipMemcpyAsync(m.quads, qb.quads, (size_t)nq * 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(mesh_t0_kernel, dim3(nblk(nq)), dim3(kMeshThreads), 0, h->stream, nq, (const int4 *)m.quads, d_pts, m.t0);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            mesh_free_one(m);
            return fail(h, SITRK_EHIP, "%s: copying the quadrangles -> %s", fn, hipGetErrorString(e));
        }
    }
    RCCHK(h->mesh_build_timer.mark(h, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->mesh_build_timer.done();
    mesh_free_one(h->mesh[mesh]);
    h->mesh[mesh] = m;
    if (nT) *nT = nt;
    if (nQ) *nQ = nq;
    if (rounds) *rounds = nr;
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_cells(sitrk_t *h, int mesh, int64_t cap, int32_t *cells, int64_t *nQ)
{
    const char *fn = "sitrk_mesh_cells";
    NEED(h, "null handle");
    RCCHK(mesh_check(h, fn, mesh, true));
    if (!nQ) return fail(h, SITRK_EINVAL, "%s: null nQ", fn);
    if (cap < 0) return fail(h, SITRK_EINVAL, "%s: cap must be >= 0", fn);
    const Mesh &m = h->mesh[mesh];
    *nQ = m.nQ;
    if (m.nQ == 0 || cap < m.nQ) return SITRK_OK;
    if (!cells) return fail(h, SITRK_EINVAL, "%s: null array", fn);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(download(h, cells, m.quads, (size_t)4 * m.nQ));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_mark(sitrk_t *h, int mesh, int jrec0)
{
    const char *fn = "sitrk_mesh_mark";
    NEED(h, "null handle");
    RCCHK(mesh_check(h, fn, mesh, true));
    Mesh &m = h->mesh[mesh];
    m.jrec0 = jrec0;
    if (m.nQ == 0) return SITRK_OK;
    HIPCHK(hipSetDevice(h->device));
    pt *d_pts;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_pts, h->nP); }));
    RCCHK(deform_points_now(h, d_pts));
    hipLaunchKernelGGL(mesh_t0_kernel, dim3(nblk(m.nQ)), dim3(kMeshThreads), 0, h->stream, m.nQ, (const int4 *)m.quads, d_pts, m.t0);
    HIPCHK(hipGetLastError());
    return SITRK_OK;
}

int sitrk::mesh_deform_check(sitrk_ctx *h, const char *fn, int mesh, int jrec1)
{
    RCCHK(mesh_check(h, fn, mesh, true));
    const Mesh &m = h->mesh[mesh];
    if (jrec1 < m.jrec0) return fail(h, SITRK_EINVAL, "%s: jrec1 = %d lies before the mesh's t0 at record %d", fn, jrec1, m.jrec0);
    return SITRK_OK;
}

int sitrk::mesh_deform_core(sitrk_ctx *h, int mesh, int jrec1, bool want_out, bool want_status, bool want_stats, size_t extra,
                            MeshDeformDev *r)
{
    const Mesh &m = h->mesh[mesh];
    const int64_t nQ = m.nQ, nP = h->nP;
    const double T = (double)((int64_t)jrec1 - m.jrec0 + 1) * h->rdt;                  // one rounded product
    HIPCHK(hipSetDevice(h->device));
    const int64_t nb = nblk(nQ);
    pt *d_p1; double *d_out, *d_part, *d_stats; int8_t *d_status; char *d_extra;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        c.take(d_p1, nQ ? nP : 0); c.take(d_out, want_out ? (size_t)5 * nQ : 0); c.take(d_status, want_status ? (size_t)nQ : 0);
        c.take(d_part, want_stats ? (size_t)nb * SITRK_MESH_NSTATS : 0); c.take(d_stats, nQ ? SITRK_MESH_NSTATS : 0);
        c.take(d_extra, extra);
    }));
    *r = MeshDeformDev();
    r->extra = d_extra;
    if (nQ == 0) return SITRK_OK;
    RCCHK(h->mesh_deform_timer.begin(h));
    RCCHK(h->mesh_deform_timer.mark(h, 0));
    RCCHK(deform_points_span(h, m.jrec0, jrec1, d_p1));
    RCCHK(h->mesh_deform_timer.mark(h, 1));
    hipLaunchKernelGGL(mesh_cells_kernel, dim3((unsigned)nb), dim3(kMeshThreads), 0, h->stream, nQ, (const int4 *)m.quads, m.t0, d_p1, T, m.par,
                       want_out ? d_out : nullptr, want_status ? d_status : nullptr, want_stats ? d_part : nullptr);
    HIPCHK(hipGetLastError());
    RCCHK(h->mesh_deform_timer.mark(h, 2));
    if (want_stats) {
        hipLaunchKernelGGL(mesh_sum_kernel, dim3(1), dim3(kMeshThreads), 0, h->stream, nb, d_part, d_stats);
        HIPCHK(hipGetLastError());
    }
    RCCHK(h->mesh_deform_timer.mark(h, 3));
    h->mesh_deform_timer.done();
    r->nQ = nQ; r->quads = m.quads; r->t0 = m.t0; r->p1 = d_p1;
    r->out = want_out ? d_out : nullptr; r->status = want_status ? d_status : nullptr; r->stats = want_stats ? d_stats : nullptr;
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_deform(sitrk_t *h, int mesh, int jrec1, double *out, int8_t *status, double *stats)
{
    const char *fn = "sitrk_mesh_deform";
    NEED(h, "null handle");
    RCCHK(mesh_deform_check(h, fn, mesh, jrec1));
    if (!out && !status && !stats) return fail(h, SITRK_EINVAL, "%s: out, status and stats are all null", fn);
    if (stats)
        for (int k = 0; k < SITRK_MESH_NSTATS; k++) stats[k] = 0.0;
    const int64_t nQ = h->mesh[mesh].nQ;
    if (nQ == 0) return SITRK_OK;
    MeshDeformDev d;
    RCCHK(mesh_deform_core(h, mesh, jrec1, out != nullptr, status != nullptr, stats != nullptr, 0, &d));
    if (out) HIPCHK(download(h, out, d.out, (size_t)5 * nQ));
    if (status) HIPCHK(download(h, status, d.status, (size_t)nQ));
    if (stats) HIPCHK(download(h, stats, d.stats, (size_t)SITRK_MESH_NSTATS));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_free(sitrk_t *h, int mesh)
{
    NEED(h, "null handle");
    if (mesh < 0 || mesh >= SITRK_MESH_MAX)
        return fail(h, SITRK_EINVAL, "sitrk_mesh_free: mesh must be in 0..%d (got %d)", SITRK_MESH_MAX - 1, mesh);
    if (h->mesh[mesh].built) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));         // a mark or a deform queued on the mesh has run
        mesh_free_one(h->mesh[mesh]);
    }
    return SITRK_OK;
}

SITRK_API int sitrk_mesh_kernel_ms(sitrk_t *h, float *build_ms, float *points_ms, float *cells_ms, float *stats_ms)
{
    NEED(h, "null handle");
    if (build_ms) {
        NEED(h->mesh_build_timer.complete, "sitrk_mesh_kernel_ms: no sitrk_mesh_build has run to its end yet");
        RCCHK(h->mesh_build_timer.elapsed(h, 0, build_ms));
    }
    if (points_ms || cells_ms || stats_ms) {
        NEED(h->mesh_deform_timer.complete, "sitrk_mesh_kernel_ms: no sitrk_mesh_deform has run its kernels yet");
        float *out[3] = {points_ms, cells_ms, stats_ms};
        for (int k = 0; k < 3; k++) RCCHK(h->mesh_deform_timer.elapsed(h, k, out[k]));
    }
    return SITRK_OK;
}
