// rt_march_xsetup.inc -- block [B] of the march loop (rt_march.hip): the arithmetic of the cross-cell set-up, Helper.h:328-336 --
// where the ray stands in its cell (u, v), the refractive index there and its gradient from the four corners.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text): march_wave includes it inside
// `if (st == ST_XSETUP)`, in front of the state resets of the integrator (lim2, dzcap, r = 0, ...), which stay there; the unit
// test dm_march_xsetup_kernel (rt_devmath.hip) includes it alone, one case per lane.
//
// Reads from the including scope: px, py, mirror; the interval pair of either axis as block [A2] leaves it, ix0 / iy0 =
//   {lo, rw = 1 / (double) w} and ix1.x / iy1.x = w = (float) (hi - lo); the corner indices rounded to float f00, f10, f01,
//   f11 and their four edge differences in double dnx0, dnx1, dny0, dny1.
// Writes: n0, gxn, gyn.
// Declares (in the including block): ya, dwx, dwy, xc0, yc0, rwx, rwy, u, v.
            const float ya   = mirror ? fabsf(py) : py;
            const double dwx = (double) ix1.x, dwy = (double) iy1.x; // Helper.h:323-324
            const double xc0 = ix0.x, yc0 = iy0.x, rwx = ix0.y, rwy = iy0.y;
            const float u    = (float) div_by_recip<true>((double) px - xc0, dwx, rwx);
            const float v    = (float) div_by_recip<true>((double) ya - yc0, dwy, rwy);
            n0  = lerp2(u, v, f00, f10, f01, f11);
            gxn = (float) (div_by_recip<true>((1.0 - (double) v) * dnx0, dwx, rwx) +
                           div_by_recip<true>((double) v * dnx1, dwx, rwx));
            gyn = (float) (div_by_recip<true>((1.0 - (double) u) * dny0, dwy, rwy) +
                           div_by_recip<true>((double) u * dny1, dwy, rwy));
            if (mirror && py < 0)
                gyn = -gyn;
