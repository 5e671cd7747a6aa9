// rt_march_xsetup.inc -- block [B] of the march loop (rt_march.hip): the arithmetic of the cross-cell set-up, Helper.h:328-336 --
// where the ray stands in its cell (u, v), the refractive index there and its gradient from the four corners.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text): march_wave includes it inside
// `if (st == ST_XSETUP)`, in front of the state resets of the integrator (lim2, dzcap, r = 0, ...), which stay there; the unit
// test dm_march_xsetup_kernel (rt_devmath.hip) includes it alone, one case per lane.
//
// Reads from the including scope: the template parameter BOUNDED; px, py; G.mirror_y, the header word of the lane's length (the
//   header block [A2] ran with: a lane reaches [B] only behind an [A2] of the same G); the interval pair of either axis as
//   block [A2] leaves it, ix0 / iy0 = {lo, rw = 1 / (double) w} and ix1.x / iy1.x = w = (float) (hi - lo); the corner indices rounded to float f00, f10, f01,
//   f11 and their four edge differences in double dnx0, dnx1, dny0, dny1.
// Writes: n0, gxn, gyn.
// Declares (in the including block): ya, dwx, dwy, xc0, yc0, rwx, rwy, quot, u, v.
            const float ya   = G.mirror_y != 0 ? fabsf(py) : py;
            const double dwx = (double) ix1.x, dwy = (double) iy1.x; // Helper.h:323-324
            const double xc0 = ix0.x, yc0 = iy0.x, rwx = ix0.y, rwy = iy0.y;
            // BOUNDED: no sign copy on the six quotients (div_by_recip_pos0, rt_math.h: the same double unless the dividend
            // is -0, then +0 for -0).  Under the ranges of the short forms no gradient quotient of a non-zero dividend
            // underflows (rt_plan.hip, "no quotient of the cross-cell set-up underflows"): a zero one has a zero dividend.
            // u, v: the dividend is a rounded difference, -0 only for px = -0 (ya = -0) over a first interval that starts
            // at +0; such a u enters n0 beside 1.0f * f00 with f00 >= 0.25, and the gradient as the zero factor of one
            // term.  The gradient: a sum of two quotients is -0 only if both are.  A zero term beside a non-zero one is
            // absorbed; two zero terms have dividends that are zeros, and the corner differences are rounded differences
            // of indices of at least 0.25: +0 where the corners are equal, never -0.  So (1 - v) dnx0 is -0 only for
            // v = 1 with dnx0 < 0 or for v > 1 with dnx0 = +0, and v dnx1 only for v < 0 with dnx1 = +0 or for a zero v
            // of the sign opposite to dnx1's: the first takes v >= 1, the second v <= 0 -- never both, and the sum is +0
            // with or without the copy.  The generic instance keeps the copies: with corner differences in the double
            // subnormals a quotient underflows to -0 beside a -0 dividend (tests/test_gpu_march_blocks.py,
            // setup/tiny_differences, has two such cases in 20 009).  tests/test_gpu_march_zero_signs.py runs both forms.
            auto quot = [](double a, double b, double y) { return BOUNDED ? div_by_recip_pos0(a, b, y) : div_by_recip<true>(a, b, y); };
            const float u    = (float) quot((double) px - xc0, dwx, rwx);
            const float v    = (float) quot((double) ya - yc0, dwy, rwy);
            n0  = lerp2(u, v, f00, f10, f01, f11);
            gxn = (float) (quot((1.0 - (double) v) * dnx0, dwx, rwx) + quot((double) v * dnx1, dwx, rwx));
            gyn = (float) (quot((1.0 - (double) u) * dny0, dwy, rwy) + quot((double) u * dny1, dwy, rwy));
            if ((G.mirror_y != 0) & (py < 0))
                gyn = -gyn;
