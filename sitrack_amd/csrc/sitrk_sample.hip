// sitrk_sample.hip -- model fields sampled along the trajectories (sitrk_sample_slot, sitrk_sample_fields): an EXTRA the
// reference does not have.  Kept in its own translation unit so that the device code of sitrk.hip stays as it is.
//
// One kernel, sample_fields_kernel<FT>: one buoy per lane over the CELL-SORTED state, so that a wave's gathers fall in a few
// rows of each field; the results go out in the caller's order through perm.  Which buoys are sampled:
//   mode AFTER  the buoys that stepped at jrec -- stepped_at() of sitrk_internal.h, the rule of fetch_record_kernel;
//   mode ENTER  the buoys alive before the step of jrec whose window opens at jrec (every alive buoy without windows).
// The value is the bit pattern found at [jT,iT]: no interpolation, no land masking (NaN payloads survive), -9999 elsewhere.
// A buoy that must be sampled and whose cell lies outside the box the fields cover is counted through a vector atomic; the
// driver at the end of this file turns a non-zero count into SITRK_EINVAL.
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sitrk_internal.h"

namespace sitrk {

namespace {

constexpr int kSmpThreads = 256;
constexpr int kSmpMaxFields = SITRK_SAMPLE_MAX_FIELDS;     // the field pointers travel as kernel arguments

// values move as integers of the element's width: a select between floats could quieten a signalling NaN
template <typename FT> struct BitsOf;
template <> struct BitsOf<float>  { typedef uint32_t type; static constexpr uint32_t fill = 0xc61c3c00u; };             // -9999.0f
template <> struct BitsOf<double> { typedef uint64_t type; static constexpr uint64_t fill = 0xc0c3878000000000ull; };   // -9999.0

template <typename FT>
struct SampleArgs {
    const typename BitsOf<FT>::type *field[kSmpMaxFields];   // element (j0, i0) of each field
    typename BitsOf<FT>::type *out;                          // (nf, n), caller order
    int64_t ld;                                              // elements between consecutive rows of a field
    int nf, j0, i0, nj, ni;                                  // the box [j0, j0+nj) x [i0, i0+ni) the fields cover
    int jrec, mode;
};

template <typename FT>
__global__ __launch_bounds__(kSmpThreads) void sample_fields_kernel(int64_t n, BuoyState st, bool windowed, SampleArgs<FT> a,
                                                                    unsigned long long *__restrict__ outside)
{
    typedef typename BitsOf<FT>::type BT;
    const int64_t s = (int64_t)blockIdx.x * kSmpThreads + threadIdx.x;
    if (s >= n) return;
    const int32_t o = st.perm[s];
    const int32_t c = st.cell[s];
    bool take;
    if (a.mode == SITRK_SAMPLE_AFTER) {
        take = stepped_at(st, s, c, a.jrec, windowed);
    } else {
        take = c >= 0;
        if (windowed) take = take && st.win[s].x == a.jrec;
    }
    const int dj = cell_j(c) - a.j0, di = cell_i(c) - a.i0;
    if (take && !((unsigned)dj < (unsigned)a.nj && (unsigned)di < (unsigned)a.ni)) {
        atomicAdd(outside, 1ull);
        take = false;
    }
    const int64_t at = (int64_t)dj * a.ld + di;
    BT v[kSmpMaxFields];
#pragma unroll
    for (int f = 0; f < kSmpMaxFields; f++)
        if (f < a.nf) v[f] = take ? a.field[f][at] : BitsOf<FT>::fill;
#pragma unroll
    for (int f = 0; f < kSmpMaxFields; f++)
        if (f < a.nf) a.out[(int64_t)f * n + o] = v[f];
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kSmpThreads - 1) / kSmpThreads); }

}  // namespace

}  // namespace sitrk

using namespace sitrk;

static inline size_t smp_elem(int dtype) { return dtype == SITRK_F64 ? 8 : 4; }

// What both entry points check first
static int sample_check(sitrk_ctx *h, const char *fn, int mode, const void *out)
{
    NEED(h, "null handle");
    if (!h->st[0].pos || h->nP == 0) return fail(h, SITRK_EINVAL, "%s: no buoys (call sitrk_set_buoys first)", fn);
    if (mode != SITRK_SAMPLE_AFTER && mode != SITRK_SAMPLE_ENTER)
        return fail(h, SITRK_EINVAL, "%s: mode must be SITRK_SAMPLE_AFTER (0) or SITRK_SAMPLE_ENTER (1), got %d", fn, mode);
    if (!out) return fail(h, SITRK_EINVAL, "%s: null output", fn);
    return SITRK_OK;
}

// The driver: nf device fields, each addressed at element (j0, i0) with rows ld elements apart, sampled into d_out (nf, nP) on
// the compute stream behind the stepping already queued; d_out -> out, then the call waits for the compute stream only.
static int sample_run(sitrk_ctx *h, const char *fn, int jrec, int mode, int nf, int dtype, const void *const *d_fields, int j0, int j1,
                      int i0, int i1, int64_t ld, void *d_out, void *out)
{
    const int64_t nP = h->nP;
    HIPCHK(hipMemsetAsync(h->counter, 0, sizeof(unsigned long long), h->stream));
    if (dtype == SITRK_F64) {
        SampleArgs<double> a;
        for (int f = 0; f < kSmpMaxFields; f++) a.field[f] = (const uint64_t *)d_fields[f < nf ? f : 0];
        a.out = (uint64_t *)d_out; a.ld = ld; a.nf = nf; a.j0 = j0; a.i0 = i0; a.nj = j1 - j0; a.ni = i1 - i0; a.jrec = jrec; a.mode = mode;
        hipLaunchKernelGGL((sample_fields_kernel<double>), dim3(nblk(nP)), dim3(kSmpThreads), 0, h->stream, nP, h->st[h->cur], h->windowed, a,
                           h->counter);
    } else {
        SampleArgs<float> a;
        for (int f = 0; f < kSmpMaxFields; f++) a.field[f] = (const uint32_t *)d_fields[f < nf ? f : 0];
        a.out = (uint32_t *)d_out; a.ld = ld; a.nf = nf; a.j0 = j0; a.i0 = i0; a.nj = j1 - j0; a.ni = i1 - i0; a.jrec = jrec; a.mode = mode;
        hipLaunchKernelGGL((sample_fields_kernel<float>), dim3(nblk(nP)), dim3(kSmpThreads), 0, h->stream, nP, h->st[h->cur], h->windowed, a,
                           h->counter);
    }
    HIPCHK(hipGetLastError());
    unsigned long long bad = 0;
    HIPCHK(download(h, &bad, h->counter, 1));
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)nf * nP * smp_elem(dtype), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (bad)
        return fail(h, SITRK_EINVAL, "%s: %llu buoy(s) to sample at record %d have their host cell outside the box rows [%d,%d) x columns [%d,%d)",
                    fn, bad, jrec, j0, j1, i0, i1);
    return SITRK_OK;
}

SITRK_API int sitrk_sample_slot(sitrk_t *h, int slot, int jrec, int mode, int field, void *out)
{
    const char *fn = "sitrk_sample_slot";
    RCCHK(sample_check(h, fn, mode, out));
    if (!h->slabs) return fail(h, SITRK_EINVAL, "%s: call sitrk_alloc_records first", fn);
    if (slot < 0 || slot >= h->nslots) return fail(h, SITRK_EINVAL, "%s: slot out of range", fn);
    if (field < 0 || field > 2) return fail(h, SITRK_EINVAL, "%s: field must be 0 (u), 1 (v) or 2 (siconc), got %d", fn, field);
    // the box the library remembers for the slot: nothing outside it is ever read, whatever the memory holds
    const int j0 = h->slot_row_lo[slot], j1 = h->slot_row_hi[slot], i0 = h->slot_col_lo[slot], i1 = h->slot_col_hi[slot];
    if (j0 >= j1 || i0 >= i1) return fail(h, SITRK_EINVAL, "%s: slot %d holds no record", fn, slot);
    HIPCHK(hipSetDevice(h->device));
    const size_t es = smp_elem(h->dtype);
    char *d_out;
    RCCHK(carve_scratch(h, [&](Carver &c) { c.take(d_out, (size_t)h->nP * es); }));
    const void *base = nullptr;
    RCCHK(slot_order_read(h, slot, field, &base));
    const void *d_field = (const char *)base + ((size_t)j0 * h->Ni + i0) * es;
    return sample_run(h, fn, jrec, mode, 1, h->dtype, &d_field, j0, j1, i0, i1, h->Ni, d_out, out);
}

SITRK_API int sitrk_sample_fields(sitrk_t *h, int jrec, int mode, int nf, int dtype, int j0, int j1, int i0, int i1,
                                  const void *const *boxes, int64_t ld, void *out)
{
    const char *fn = "sitrk_sample_fields";
    RCCHK(sample_check(h, fn, mode, out));
    if (nf < 1 || nf > kSmpMaxFields) return fail(h, SITRK_EINVAL, "%s: nf must be in 1..%d, got %d", fn, kSmpMaxFields, nf);
    if (dtype != SITRK_F32 && dtype != SITRK_F64) return fail(h, SITRK_EINVAL, "%s: dtype must be SITRK_F32 or SITRK_F64", fn);
    NEED(h->geo, "sitrk_sample_fields: call sitrk_set_grid first");
    if (!(j0 >= 0 && j0 < j1 && j1 <= h->Nj && i0 >= 0 && i0 < i1 && i1 <= h->Ni))
        return fail(h, SITRK_EINVAL, "%s: box rows [%d,%d) x columns [%d,%d) empty or outside the %d x %d grid", fn, j0, j1, i0, i1, h->Nj, h->Ni);
    const int64_t nj = j1 - j0, ni = i1 - i0;
    if (ld < ni) return fail(h, SITRK_EINVAL, "%s: ld = %lld is less than the %lld columns of the box", fn, (long long)ld, (long long)ni);
    NEED(boxes, "sitrk_sample_fields: null boxes");
    for (int f = 0; f < nf; f++)
        if (!boxes[f]) return fail(h, SITRK_EINVAL, "%s: field %d is a null pointer", fn, f);
    HIPCHK(hipSetDevice(h->device));
    const size_t es = smp_elem(dtype);
    // device copies of the boxes, packed (rows ni elements apart), in the transient scratch: reused by the next call
    char *d_box[kSmpMaxFields] = {nullptr}, *d_out;
    RCCHK(carve_scratch(h, [&](Carver &c) {
        for (int f = 0; f < nf; f++) c.take(d_box[f], (size_t)nj * ni * es);
        c.take(d_out, (size_t)nf * h->nP * es);
    }));
    const void *d_fields[kSmpMaxFields] = {nullptr};
    for (int f = 0; f < nf; f++) {
        if (ld == ni)
            HIPCHK(hipMemcpyAsync(d_box[f], boxes[f], (size_t)nj * ni * es, hipMemcpyHostToDevice, h->stream));
        else
            HIPCHK(hipMemcpy2DAsync(d_box[f], (size_t)ni * es, boxes[f], (size_t)ld * es, (size_t)ni * es, (size_t)nj, hipMemcpyHostToDevice,
                                    h->stream));
        d_fields[f] = d_box[f];
    }
    return sample_run(h, fn, jrec, mode, nf, dtype, d_fields, j0, j1, i0, i1, ni, d_out, out);
}
