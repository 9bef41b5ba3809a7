// pose_lm_round.inc - the one copy of the speculative Levenberg-Marquardt round of pose_opt.hip::po_run and
// pose_stereo.hip::ps_run: lambda0 from the six diagonal sums, then the iterations.  Included as TEXT inside the round loop of
// each, behind the evaluation at the round's start pose, so that it is compiled exactly where and as it was written in each
// file: it carries no contraction pragma, and its scalar arithmetic - the gain-ratio denominator, the gain ratio, the accept
// factor - takes the state of the including file at that place (pose_opt.hip: the compiler's default; pose_stereo.hip:
// contract(off)).  A force-inlined template over a model object was built first and not kept: optimised as a function of its
// own before it is inlined, it handed po_apply_update's sums to the instruction selector with operands commuted, other
// multiply-adds were fused under pose_opt.hip's default, and 28 accepted steps became 27 on a 200-edge frame
// (DESIGN.md 4v).
//
// The including function provides
//   lm          po_lm_shared&: the candidate poses and the per-trial scalars
//   tid, prm.iterations, nactive
//   cur, cand   double*: the sums at the current pose / where the next trial's go           (updated)
//   T           const double*: the current pose                                             (updated)
//   p, accepted int: the candidate buffer of the next iteration; accepted steps             (updated)
//   PO_LM_EVALUATE(T, out)        one block-wide evaluation at pose T: out[0..20] = upper H, [21..26] = b, [27] = robust cost
//   PO_LM_COSTS(Tk, solved, out)  the robust costs at PO_SPEC poses in one pass
//   PO_LM_CURRENT()               the evaluation just made is now the one of the current pose (the monocular file swaps its
//                                 two chi2 buffers; the stereo file does nothing)
        double lambda, ni = 2.0;
        {
            double dmax = 0.0;
            const int diag[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
            for (int i = 0; i < 6; i++) dmax = fmax(dmax, cur[diag[i]]);
            lambda = 1e-5 * fmax(dmax, 1e-12);          // tau * max diagonal
        }
        for (int it = 0; it < prm.iterations && nactive > 0; it++) {
            // ---- the ten trials of this iteration are PROPOSED together.  A trial that is turned down changes nothing but
            // the damping (lambda *= ni, ni *= 2), so the candidates of all ten trials are known in advance: lane j of
            // wave 0 solves with the damping trial j would meet and builds its pose - ten solves in the instruction stream
            // of one.  Trial 0 is then evaluated in full (cost, H, b); only when it is turned down does ONE more pass give
            // the costs of trials 1..9, and they are walked in order: the first one the sequential loop would have accepted
            // is accepted, with the damping that loop would have had.  g2o's schedule ends every round on ten rejected
            // trials (maxTrialsAfterFailure): ten sequential solve + evaluation pairs (38 us of a 67 us round at 200
            // edges) become one solve and two passes.
            double* cands = lm.pose[p];
            if (tid < PO_TRIALS) {
                double lam = lambda, n2 = ni;
                for (int k = 0; k < tid; k++) { lam *= n2; n2 *= 2.0; }
                double dx[6];
                const bool ok_j = po_solve(cur, cur + 21, lam, dx);
                double sc = 1e-3;
                for (int i = 0; i < 6; i++) sc += dx[i] * (lam * dx[i] - cur[21 + i]);
                lm.solved_k[tid] = ok_j ? 1 : 0;
                if (ok_j) { po_apply_update(dx, T, cands + 12 * tid); lm.scale_k[tid] = sc; }
            }
            __syncthreads();
            const int solved = lm.solved_k[0];          // read now: the next iteration's proposals overwrite them
            const double scale = lm.scale_k[0];
            if (solved) PO_LM_EVALUATE(cands, cand);
            const double rho0 = solved ? (cur[27] - cand[27]) / scale : -1.0;
            if (solved && rho0 > 0.0 && isfinite(cand[27])) {
                { double* t = cur; cur = cand; cand = t; }
                PO_LM_CURRENT();
                T = cands;
                p ^= 1;
                const double gq = 2.0 * rho0 - 1.0;
                lambda *= fmax(1.0 / 3.0, fmin(1.0 - gq * gq * gq, 2.0 / 3.0));
                ni = 2.0;
                accepted++;
                continue;
            }
            lambda *= ni;
            ni *= 2.0;
            if (solved && !isfinite(lambda)) break;     // (an unsolvable system never ends the iteration by itself)
            // ---- trial 0 was turned down: the costs of trials 1..9 in one pass, walked in order
            PO_LM_COSTS(cands + 12, lm.solved_k + 1, lm.cost_k);
            int taken = -1;
            for (int j = 0; j < PO_SPEC; j++) {
                if (lm.solved_k[j + 1]) {
                    const double rho = (cur[27] - lm.cost_k[j]) / lm.scale_k[j + 1];
                    if (rho > 0.0 && isfinite(lm.cost_k[j])) {
                        const double gq = 2.0 * rho - 1.0;
                        lambda *= fmax(1.0 / 3.0, fmin(1.0 - gq * gq * gq, 2.0 / 3.0));
                        ni = 2.0;
                        taken = j + 1;
                        break;
                    }
                }
                lambda *= ni;
                ni *= 2.0;
                if (lm.solved_k[j + 1] && !isfinite(lambda)) break;
            }
            if (taken < 0) break;                       // ten trials turned down (or the damping overflowed): the round's iterations end
            accepted++;
            T = cands + 12 * taken;
            p ^= 1;
            PO_LM_EVALUATE(T, cur);                     // H, b, cost at the accepted pose
            PO_LM_CURRENT();
        }
