// rt_march_step.inc -- block [C] of the march loop (rt_march.hip): one integrator step, Helper.h:281-311, and the loop
// condition of Helper.h:279-280 evaluated behind it -- the index at the ray's place, the three quotients by it, the
// tiny-dividend guard, the step size in its three forms (IEEE; BOUNDED: the short division sequences and the NaN-dropping
// minimum; MARCH_OPT_PRUNE: divisions that cannot set the step skipped wave by wave), the Taylor update, renormalise, hsum.
//
// A fragment of a function body, not a header (rt_tile_rec.inc says why text): march_wave includes it inside
// `if (st == ST_STEP) { ...; bool run; { <here> } if (!run) ... }`; the unit test dm_march_step_kernel (rt_devmath.hip)
// includes it alone, one case per lane.  It takes wave-level decisions (__ballot): every lane of the wave must arrive.
//
// Reads from the including scope: the template parameters BOUNDED and OPT; n0, gxn, gyn, lim0, lim1, lim2, dzcap;
//   P.c_h1, P.c_h3 (c * 0.1f, c * 0.05f); diag, whose tiny_dividend(), prune(k) and tick(0) it calls -- the product's
//   MarchDiag, or a counting stand-in.
// Reads and writes: rx, ry, rz, sx, sy, sz, hsum.
// Writes: n, run.
// Declares (in the including block): rn, a0, t, qx, qy, fx, fy, fz, h, ht, F1, F2, c1, c2 and the candidates of its
//   branches; defines the macro RT_FDIV.
                n        = n0 + rx * gxn + ry * gyn;
#ifdef RT_ABL_FASTDIV
#define RT_FDIV(a, b) ((a) * __builtin_amdgcn_rcpf(b))
#else
#define RT_FDIV(a, b) ((a) / (b))
#endif
                // one IEEE division, three exact quotients
                const float rn = BOUNDED ? fdiv_one_nr(n) : RT_FDIV(1.0f, n);
                float a0 = sx * gxn + sy * gyn + 1e-12f;
                // (BOUNDED: a0 is never -0 -- x + 1e-12f is +0 or non-zero -- and rn > 0, so the corrected
                // quotient has the sign of a0 without the sign copy)
                float t  = BOUNDED ? fmaf(fmaf(-n, a0 * rn, a0), rn, a0 * rn) : div_by_recip_signed(a0, n, rn);
                // (qx, qy keep their sign copy: gyn = -gyn of a mirrored cell makes a -0 gradient, and with sx = -0 and
                // t < 0 the sign of a zero qx decides between sx = -0 and +0 after the step)
                float qx = div_by_recip_signed(gxn, n, rn);
                float qy = div_by_recip_signed(gyn, n, rn);
#ifndef RT_ABL_NOGUARD
                // div_by_recip needs a true division for non-zero dividends below 1e-29 (rt_math.h).  One
                // wave-uniform test covers the three quotients: the smallest magnitude of the dividends is
                // below the bound only where a lane holds an exact zero (index gradient of a uniform
                // region; the quotient 0 is right as it is) or, once in a blue moon, such a dividend.
                // (Such a gradient, that is: a0 = x + 1e-12f is zero or at least 2^-64 in magnitude -- a sum that small
                // is exact -- so the branch of a0 below is never taken, tests/test_march_blocks_host.py.)
                if (__ballot(fminf(fminf(fabsf(a0), fabsf(gxn)), fabsf(gyn)) < 1e-29f) != 0ull) {
                    diag.tiny_dividend();
                    if (fabsf(a0) < 1e-29f && a0 != 0.0f) {
                        asm volatile("" : "+v"(a0));
                        t = a0 / n;
                    }
                    if (fabsf(gxn) < 1e-29f && gxn != 0.0f) {
                        float g = gxn;
                        asm volatile("" : "+v"(g));
                        qx = g / n;
                    }
                    if (fabsf(gyn) < 1e-29f && gyn != 0.0f) {
                        float g = gyn;
                        asm volatile("" : "+v"(g));
                        qy = g / n;
                    }
                }
#endif
                float fx = qx - sx * t;
                float fy = qy - sy * t;
                float fz = -sz * t;
                float h;
                if (BOUNDED && (OPT & MARCH_OPT_PRUNE)) {
                    // The same candidates, but a division is executed only where its quotient can matter.  Four of the
                    // five candidates are quotients num / den with num >= 0, den >= 0, and the step is their minimum
                    // with dzcap: a candidate whose exact quotient exceeds dzcap rounds to a float >= dzcap (or, where the
                    // short sequence is out of its range, to something huge, infinite or NaN that the minimum passes
                    // over, see below), so leaving it out of the minimum returns the same float.  Sufficient, without a
                    // division: p = RN(RN(K dzcap) den) < num with K = 1.00002f.  The two products lose at most 2^-24
                    // each, so p >= K (1 - 2^-24)^2 dzcap den > dzcap den (K - 1 = 168 x 2^-23 against the 2^-23 needed)
                    // and num > p gives num / den > dzcap.  (K = 1.0f would do as well: RN(dzcap den) is then the float
                    // nearest the exact product, so a float above it is at least the product; the margin costs the divisions
                    // of the candidates within 168 ulp above dzcap, tests/test_march_blocks_host.py.)  A product that lands in the subnormal range (absolute
                    // error 2^-150) could only mislead a numerator below 2^-125: those of h1 and h4 are at least
                    // 5e-12 (c_h3 >= 1e-8), and for h2 it takes |sz| dzcap < 2^-125 while num >= 2^-24 lim2, i.e.
                    // num / |sz| > 2^101 lim2 dzcap > dzcap (lim2 >= 5e-6 dz / 3 >= 1e-18 under the BOUNDED ranges).
                    // A comparison with a NaN or against den = inf is false: that candidate is divided as before.
                    // K is small enough to keep pruning h2 right after a dzcap step, where h2 / dzcap is about
                    // 1.0001 / (1.00001 |sz|) >= 1.00008.  The decision is taken for the wave (one scalar branch per
                    // candidate or pair of candidates): on the 6.4 M-ray stand-in dzcap sets 63 % of the steps, h3 35 %, h4 0.8 %, h2 0.6 %, h1
                    // none (DESIGN.md 4.1), so h3 is always divided.
                    const float kd = 1.00002f * dzcap;
                    const float at = fabsf(t), az = fabsf(sz);
                    const float n2 = 1.0001f * (lim2 - fabsf(rz));
                    const float n4 = P.c_h3 * (fabsf(sy) + 5e-4f), d4 = fabsf(fy) + 1e-8f;
                    h = fmin_nan_drop(fdiv_nr(P.c_h3 * (fabsf(sx) + 5e-4f), (fabsf(fx) + 1e-8f)), dzcap);
                    diag.prune(3);
                    if (__ballot(!(P.c_h1 > kd * at)) != 0ull) {
                        h = fmin_nan_drop(fdiv_nr(P.c_h1, at), h);
                        diag.prune(0);
                    }
                    // h2 and h4 behind ONE branch, their two divisions interleaved when it is taken: a branch each ran the
                    // stand-in 1.6 % faster than none but 2 - 3 % slower on launches of a few rays per lane, whose waves
                    // wait on their own dependency chain and not on the issue slots (profiles/step_prune_ab.txt); merged
                    // it is 2.0 % on the stand-in, and the small launches go without it (rt_launch.hip)
                    if (!(OPT & MARCH_OPT_PRUNE_H24) || __ballot(!(n2 > kd * az) | !(n4 > kd * d4)) != 0ull) {
                        h = fmin_nan_drop(fmin_nan_drop(fdiv_nr(n2, az), fdiv_nr(n4, d4)), h);
                        diag.prune(1);
                    }
                } else if (BOUNDED) {
                    // The step candidates (Helper.h:288-297) without the range bookkeeping of an IEEE division
                    // (fdiv_nr, rt_math.h): exact wherever a candidate can be the minimum; a candidate that the
                    // short sequence gets wrong is huge, infinite or NaN on both paths (its true value is above
                    // dzcap), and the NaN-dropping minimum below passes over it as the `<` chain passes over +inf.
                    const float h1 = fdiv_nr(P.c_h1, fabsf(t)); // c * 0.1f / |t|
                    const float h2 = fdiv_nr(1.0001f * (lim2 - fabsf(rz)), fabsf(sz));
                    const float h3 = fdiv_nr(P.c_h3 * (fabsf(sx) + 5e-4f), (fabsf(fx) + 1e-8f)); // c * 0.05f * ...
                    const float h4 = fdiv_nr(P.c_h3 * (fabsf(sy) + 5e-4f), (fabsf(fy) + 1e-8f));
                    h = fmin_nan_drop(fmin_nan_drop(h1, dzcap), fmin_nan_drop(h2, fmin_nan_drop(h3, h4)));
                } else {
                    h        = RT_FDIV(P.c_h1, fabsf(t)); // c * 0.1f / |t|
                    h        = h < dzcap ? h : dzcap;
                    float h2 = RT_FDIV(1.0001f * (lim2 - fabsf(rz)), fabsf(sz));
                    float h3 = RT_FDIV(P.c_h3 * (fabsf(sx) + 5e-4f), (fabsf(fx) + 1e-8f)); // c * 0.05f * ...
                    float h4 = RT_FDIV(P.c_h3 * (fabsf(sy) + 5e-4f), (fabsf(fy) + 1e-8f));
                    h        = h < h2 ? h : h2;
                    h        = h < h3 ? h : h3;
                    h        = h < h4 ? h : h4;
                }
                float ht = h * t;
                float F1, F2; // 1 - ht / 3 + ht^2 / 12 and 1 - ht / 2 + ht^2 / 6 (rt_math.h)
                step_factors(ht, F1, F2);
                float c1 = 0.5f * h * h * F1;
                rx += sx * h + c1 * fx;
                ry += sy * h + c1 * fy;
                rz += sz * h + c1 * fz;
                float c2 = h * F2;
                sx += c2 * fx;
                sy += c2 * fy;
                sz += c2 * fz;
                renormalise(sx, sy, sz);
                hsum += h;
                diag.tick(0);
                // (double)|n - n0| < 0.05 (Helper.h:280) <=> |n - n0| < 0.05f: 0.05f is the smallest float above 0.05
                // (MARCH_OPT_NO_NTEST: the last test is known to hold, rt_plan.hip "the largest index change a step can see")
                run = (fabsf(rx) < lim0) & (fabsf(ry) < lim1) & (fabsf(rz) < lim2);
                if (!(BOUNDED && (OPT & MARCH_OPT_NO_NTEST)))
                    run = run & (fabsf(n - n0) < 0.05f);
