// rt_blob_pack.h -- host-side packing of one length of the march blob (rt_device.h: BlobGain, Interval, Node).
//
// rt_hip_plan_create (rt_plan.hip) packs every length with it; the unit test of the march's cell set-up (rt_devmath.hip,
// rt_devmath_march_cell) packs its test grids with the same function, so that the device test reads the product's records and
// not a restatement of them.  Host code only.
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

#include "rt_device.h"

namespace rt {

// Appends the interval records of both axes and the fused corner nodes of one length to `blob` and writes the length's header
// into slot `i` of the header table at the start of the blob (the caller has sized it: BlobGain[N], 16-byte aligned).  Returns
// the header.  tiny_spacing / bad_index are set (never cleared) when a grid is not strictly increasing with a spacing of at
// least 1e-30, or an index of refraction is not finite as a float: the caller refuses such tables.
inline BlobGain blob_pack_length(std::vector<unsigned char> &blob, size_t i, int Nx, int Ny, const double *x, const double *y,
                                 const double *n, const float *g0, const float *E0, bool &tiny_spacing, bool &bad_index)
{
    const size_t npix = (size_t) Nx * (size_t) Ny;
    BlobGain h;
    memset(&h, 0, sizeof(h));
    h.lo_x     = (float) x[0]; // Helper.h:445-448
    h.hi_x     = (float) x[Nx - 1];
    h.lo_y     = (float) y[0];
    h.hi_y     = (float) y[Ny - 1];
    h.mirror_y = 0;
    if (h.lo_y >= 0) { // Helper.h:449-453
        h.lo_y     = -h.hi_y;
        h.mirror_y = 1;
    }
    h.Nx  = Nx;
    h.Ny  = Ny;
    h.x0f = (float) x[0];
    h.y0f = (float) y[0];
    const double ihx = (double) (Nx - 1) / (x[Nx - 1] - x[0]);
    const double ihy = (double) (Ny - 1) / (y[Ny - 1] - y[0]);
    h.inv_hxf        = std::isfinite(ihx) && fabs(ihx) < 1e30 ? (float) ihx : 0.0f;
    h.inv_hyf        = std::isfinite(ihy) && fabs(ihy) < 1e30 ? (float) ihy : 0.0f;
    // per-interval records of both axes (entry 0 unused)
    auto put_intervals = [&](const double *gp, int n, bool mirrored) {
        const int off = (int) blob.size();
        blob.resize(blob.size() + sizeof(Interval) * (size_t) n);
        Interval *iv = reinterpret_cast<Interval *>(blob.data() + off);
        memset(iv, 0, sizeof(Interval) * (size_t) n);
        for (int k = 1; k < n; k++) {
            const double lo = gp[k - 1], hi = gp[k], hk = hi - lo;
            if (!(hk >= 1e-30)) // see rt_math.h, div_by_recip<TINY_OK>; and the integrator's step limits
                tiny_spacing = true; // 0.1f * (float) hk must be positive (rt_march.hip, block [C])
            iv[k].lo   = lo;
            iv[k].hi   = hi;
            iv[k].rh   = 1.0 / hk;
            iv[k].rw   = 1.0 / (double) (float) hk;
            iv[k].w    = (float) hk;
            iv[k].b_lo = (float) (lo - 0.1 * hk);
            iv[k].b_hi = (float) (hi + 0.1 * hk);
            if (mirrored && k == 1)
                iv[k].b_lo = -iv[k].b_hi;
        }
        return off;
    };
    h.off_ix   = put_intervals(x, Nx, false);
    h.off_iy   = put_intervals(y, Ny, h.mirror_y != 0);
    h.off_node = (int) blob.size();
    blob.resize(blob.size() + sizeof(Node) * npix);
    Node *nd = reinterpret_cast<Node *>(blob.data() + h.off_node);
    for (size_t c = 0; c < npix; c++) { // the three gathered quantities fused per grid point
        // (the reference's integrator loop would never advance: Helper.h:279-280.  The march rounds the index to float, block
        // [A2]: an index that is finite as a double and infinite as a float is no better than an infinite one)
        if (!std::isfinite((float) n[c]))
            bad_index = true;
        nd[c].n  = n[c];
        nd[c].g0 = g0[c];
        nd[c].E0 = E0 ? E0[c] : 0.0f;
    }
    memcpy(blob.data() + sizeof(BlobGain) * i, &h, sizeof(h));
    return h;
}

} // namespace rt
