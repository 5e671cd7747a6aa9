// rt_march_cell.inc -- block [A2] of the march loop (rt_march.hip): the escape test and the cell set-up, Helper.h:465-497 --
// whether the ray has left the plasma box or turned too far from z; otherwise which cell it stands in (a float guess, verified
// against the interval's own coordinates, bisection when it fails), the two interval records and four corner nodes of that
// cell, g0 and E0 at the ray, and whether a cross-cell iteration happens at all.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text): march_wave includes it inside
// `if (in_seg)` (a lane in ST_CELL whose ray has not escaped), behind the sub-segment commit [A1], which stays there; the unit test dm_march_cell_kernel
// (rt_devmath.hip) includes it alone, one case per lane.
//
// Reads from the including scope: px, py, sz, z, z_stop; G, the BlobGain header of the lane's length, with lds_base already added
//   to its three offsets off_ix, off_iy, off_node (march_blob_header, rt_march.hip: once per header load, not once per gather);
//   tab, the march blob (global memory, or LDS when LDS_TAB) and lds_base, its LDS address (0 unless LDS_TAB; the ds_read_b128
//   gather addresses LDS by G's offsets as they are); use_emis; the template parameter LDS_TAB; diag (tick).
// Writes: st = ST_ESC for a ray that has escaped (its slot is committed by [A1] in the next iteration), or else c00, the lane state ix0, ix1, iy0, iy1 = {lo, rw}, {w, b_lo, b_hi, -} of
//   either axis, the corner indices as floats f00, f10, f01, f11 and their edge differences dnx0, dnx1, dny0, dny1, g0, E0,
//   pz = zc = path = 0, dzrem, and st = ST_XSETUP -- or, with no cross-cell iteration, the closed cell step: z, gacc, eacc,
//   cell_last, steps (st stays ST_CELL).
// Declares (in the including block): ivx, ivy, tx, ty, q00, q10, q01, q11, gather, node_n, ya, pxd, yad, k1, k2, ok, n00, n10,
//   n01, n11, u, v.
                // [A2] escape test + cell setup (Helper.h:465-497)
                // (double)(sz*sz) < 0.01 (Helper.h:466) <=> sz*sz <= 0.01f: 0.01f is the largest float below 0.01
                if ((px < G.lo_x) | (px > G.hi_x) | (py < G.lo_y) | (py > G.hi_y) | (sz * sz <= 0.01f)) {
                    st = ST_ESC; // its slot is committed by [A1] next iteration
                } else {
                    const Interval *ivx = reinterpret_cast<const Interval *>(tab + ((unsigned) G.off_ix - lds_base));
                    const Interval *ivy = reinterpret_cast<const Interval *>(tab + ((unsigned) G.off_iy - lds_base));
                    // (records are addressed by 32-bit byte offsets from the start of the blob: no
                    // 64-bit multiplies for what is an LDS address.  Interval and node numbers are below 2^24 and the blob
                    // is below 2^31 bytes -- rt_hip_plan_create refuses anything else, RT_MARCH_MAX_NODES / RT_MARCH_MAX_BLOB
                    // in rt_device.h -- so a 24-bit multiply-add forms the offset exactly: one v_mad_u32_u24 each.)
                    // One round of gathers per cell: two 48-byte interval records and four 16-byte corner nodes (the
                    // two nodes of a grid row are neighbours), ten 16-byte reads issued together.  In the LDS variant
                    // they are written as ds_read_b128 instructions whose results ARE the lane-state registers
                    // (ix0, ix1, iy0, iy1) or are consumed where they land: left to itself the compiler reads the tail
                    // of a record as ds_read_b96 and a node as b64 + b32 + b32 (issue cost per LDS instruction: b32 /
                    // b64 5, b128 10, b96 20 VALU-equivalent ticks -- tools/ubench), and held to whole 16-byte reads
                    // by empty asm statements (round 3) it paid for them with 34 register copies per cell set-up.
                    f64x2 tx, ty;            // {hi, rh} of the two intervals
                    u32x4 q00, q10, q01, q11; // corner nodes {n (f64) | g0 | E0}
                    auto gather = [&](int k1, int k2, int c) {
                        const unsigned ox = __umul24((unsigned) k1, (unsigned) sizeof(Interval)) + (unsigned) G.off_ix;
                        const unsigned oy = __umul24((unsigned) k2, (unsigned) sizeof(Interval)) + (unsigned) G.off_iy;
                        // (a node is 16 bytes: shift-adds, v_lshl_add_u32 -- a 24-bit multiply by a power of two becomes
                        // a shift and a mask)
                        static_assert(sizeof(Node) == 16, "node offsets are formed by a shift");
                        const unsigned oa = ((unsigned) c << 4) + (unsigned) G.off_node;
                        const unsigned ob = ((unsigned) G.Nx << 4) + oa;
                        if (LDS_TAB) {
                            // (G's offsets are LDS addresses here; the reads complete inside the statement, so the
                            // compiler's own wait counters stay right)
                            asm volatile("ds_read_b128 %0, %10\n\t"
                                         "ds_read_b128 %1, %10 offset:16\n\t"
                                         "ds_read_b128 %2, %10 offset:32\n\t"
                                         "ds_read_b128 %3, %11\n\t"
                                         "ds_read_b128 %4, %11 offset:16\n\t"
                                         "ds_read_b128 %5, %11 offset:32\n\t"
                                         "ds_read_b128 %6, %12\n\t"
                                         "ds_read_b128 %7, %12 offset:16\n\t"
                                         "ds_read_b128 %8, %13\n\t"
                                         "ds_read_b128 %9, %13 offset:16\n\t"
                                         "s_waitcnt lgkmcnt(0)"
                                         : "=&v"(ix0), "=&v"(ix1), "=&v"(tx), "=&v"(iy0), "=&v"(iy1), "=&v"(ty), "=&v"(q00), "=&v"(q10),
                                           "=&v"(q01), "=&v"(q11)
                                         : "v"(ox), "v"(oy), "v"(oa), "v"(ob));
                        } else {
                            const unsigned char *t = tab; // (lds_base = 0: 64-bit base + 32-bit offset)
                            ix0 = *reinterpret_cast<const f64x2 *>(t + ox);
                            ix1 = *reinterpret_cast<const f32x4 *>(t + ox + 16);
                            tx  = *reinterpret_cast<const f64x2 *>(t + ox + 32);
                            iy0 = *reinterpret_cast<const f64x2 *>(t + oy);
                            iy1 = *reinterpret_cast<const f32x4 *>(t + oy + 16);
                            ty  = *reinterpret_cast<const f64x2 *>(t + oy + 32);
                            q00 = *reinterpret_cast<const u32x4 *>(t + oa);
                            q10 = *reinterpret_cast<const u32x4 *>(t + oa + 16);
                            q01 = *reinterpret_cast<const u32x4 *>(t + ob);
                            q11 = *reinterpret_cast<const u32x4 *>(t + ob + 16);
                        }
                    };
                    auto node_n = [](const u32x4 &q) { return __hiloint2double((int) q.y, (int) q.x); };
                    const float ya      = G.mirror_y != 0 ? fabsf(py) : py; // (a header word, not lane state: [B] and [C] test it themselves)
                    const double pxd = (double) px, yad = (double) ya;
                    // one round of gathers on the guessed cell: two interval records, four nodes
                    int k1     = guess_interval(G.Nx, G.x0f, G.inv_hxf, px);
                    int k2     = guess_interval(G.Ny, G.y0f, G.inv_hyf, ya);
                    c00        = (k1 - 1) + __mul24(k2 - 1, G.Nx); // (a node number: both factors and the product below 2^24)
                    gather(k1, k2, c00);
                    const bool ok = ((k1 == 1) | (ix0.x < pxd)) & ((k1 == G.Nx - 1) | (tx.x >= pxd)) &
                                    ((k2 == 1) | (iy0.x < yad)) & ((k2 == G.Ny - 1) | (ty.x >= yad));
                    if (!ok) {
                        k1  = bisect_interval(ivx, G.Nx, pxd);
                        k2  = bisect_interval(ivy, G.Ny, yad);
                        c00 = (k1 - 1) + __mul24(k2 - 1, G.Nx);
                        gather(k1, k2, c00);
                    }
                    const double n00 = node_n(q00), n10 = node_n(q10), n01 = node_n(q01), n11 = node_n(q11);
                    f00       = (float) n00;
                    f10       = (float) n10;
                    f01       = (float) n01;
                    f11       = (float) n11;
                    dnx0      = n10 - n00;
                    dnx1      = n11 - n01;
                    dny0      = n01 - n00;
                    dny1      = n11 - n10;
                    // (no sign copy on the quotients, div_by_recip_pos0: it matters for a -0 dividend alone.  A rounded
                    // difference of equal numbers is +0, so the dividend is -0 only for px = -0 on a first
                    // interval that starts at +0 (a y axis that starts at 0 is mirrored: ya = |py|), and u = -0 reaches g0 and E0 as the term -0 * f10 beside
                    // 1.0f * f00: absorbed by a non-zero f00, and with f00 = +0 the sum is +0 for either sign of the term.
                    // Only a table value f00 = -0 under such a ray would give g0 or E0 the other zero, and that sign ends
                    // here: gacc and eacc start at +0 and x + -0 = x + +0 for every x but -0.
                    // tests/test_gpu_march_zero_signs.py holds the populations.)
                    const float u = (float) div_by_recip_pos0(pxd - ix0.x, tx.x - ix0.x, tx.y);
                    const float v = (float) div_by_recip_pos0(yad - iy0.x, ty.x - iy0.x, ty.y);
                    g0            = lerp2(u, v, __uint_as_float(q00.z), __uint_as_float(q10.z), __uint_as_float(q01.z),
                                          __uint_as_float(q11.z));
                    E0            = 0.0f;
                    if (use_emis) {
                        E0 = lerp2(u, v, __uint_as_float(q00.w), __uint_as_float(q10.w), __uint_as_float(q01.w),
                                   __uint_as_float(q11.w));
                        // (a compare and a select, not one maximum: v_max_f32 orders -0 below +0 and would turn an E0 of -0,
                        // which this keeps, into +0.  eacc could not tell -- the zero reaches it as a term E0 * path added to a
                        // sum that is never -0 -- but E0 itself is lane state that tests/test_gpu_march_cell.py compares with
                        // the reference bit for bit, population "table_values": E0 interpolating to -0, kept.)
                        E0 = E0 >= 0 ? E0 : 0.0f;
                    }
                    pz    = 0.0f;
                    zc    = 0.0f;
                    path  = 0.0f;
                    dzrem = z_stop - z;
                    // Helper.h:327 with zc = 0: 0.0 < 0.999 * (double) dzrem <=> dzrem > 0 (no underflow in double)
                    if ((px > ix1.y) & (px < ix1.z) & (ya > iy1.y) & (ya < iy1.z) & (dzrem > 0.0f)) {
                        st = ST_XSETUP;
                    } else {
                        // no cross-cell iteration at all: the cell step still counts (Helper.h:498-503)
                        // A rare arm -- the box b_lo .. b_hi is the cell with a margin, and dzrem > 0 for every lane that
                        // is in_seg: a position that is a NaN, or a z_stop the float z cannot stay below, reaches it; no wave
                        // of the stand-in does (profiles/march_overhead_ab.txt) -- that the compiler laid out as predicated
                        // straight-line code: its eight vector instructions issued in every pass of [A2], for no lane.  The
                        // empty statement makes the wave branch round the arm when no lane takes it (the compiler keeps
                        // the skip of a block that holds an asm statement).  The arithmetic stays, in every instance: with
                        // path = +0 the sums add g0 * 0 and E0 * 0, which are NaN for a table value that is not finite, and
                        // plan creation verifies the index tables only, not g0 and E0.
                        asm volatile("");
                        z += fabsf(pz);
                        gacc += g0 * path;
                        eacc += E0 * path;
                        cell_last = c00;
                        steps++;
                        diag.tick(2);
                    }
                }
