// bmpc_rollout_body.inl -- THE BODY of a rollout kernel, the stream loop and the tick loop inside it, once: bmpc_rollout_kernel.inl expands it in
// bmpc_stream_rollout_kernel (BMPCR_SE 0: arguments a, s, r) and in bmpc_stream_rollout_sensor_kernel (BMPCR_SE 1: a fourth argument of type NArgs).  No
// include guard.  The expanding function declares the constants EV, AU, LG, QU, TU, PL and ZLDS, RESTO; the lines under `#if BMPCR_SE` -- the sample ahead
// of the pack, the way back to the truth behind the post, the meas_hist rows -- exist in the sensor kernels only, and `!BMPCR_SE ||` ahead of a test of the
// plant table is a constant true in the others: a PL kernel without a sensor is launched with a plant table only, an SE kernel asks at run time.
// The lines under `#if BMPCR_OB` (with BMPCR_SE 1 only: bmpc_stream_rollout_observer_kernel, a fifth argument of type OArgs) -- the observer row's validation,
// stream_observe in the place of stream_sense, the sample_hist rows -- exist in the observer kernels only; the others expand the body with BMPCR_OB 0.
// Rationale of every section: the file comment of bmpc_rollout_kernel.inl.
    static_assert(BMPC_NW == 1 || ZLDS, "a team keeps the iterate in LDS");
    BMPCK_LDS double lds[BMPC_NAMESPACE::L_SIZE];
    BMPC_STRIDES(a);
    const int wv = BMPCK_WAVE;
    const bool w0 = BMPC_NW == 1 || wv == 0;      // the wave that runs the stream functions and stores the rows (a team: wave 0)
    double *sh = lds + BMPC_NAMESPACE::L_RED;
    static_assert(bmpcs::SH_LEN <= 6 * 64, "the stream functions' LDS words must fit into the solver's reduction area");
    static_assert(bmpcs::TUBE_LEN <= 6 * 64, "and so must a tube row");
    static_assert(bmpcs::LSH_LEN + bmpcs::LOG_STAGE + 4 <= 6 * 64, "and the log's LDS words with one stage row and its trailer behind them");
    const int TRN = bmpcs::tr_len(a.N);
    const double nan_ = __builtin_nan("");
    for (int b = BMPCK_BLOCK; b < a.B; b += BMPCK_GRID) {
        BMPC_STREAM_SLICES(a, s, b);
        long long busy = 0;      // counts of the 100 MHz clock spent in the stream's solves
        int t = 0;
        if (EV && !QU) { if (r.replan_info && BMPCK_LANE == 0) r.replan_info[b] = -1; }
        if (QU) {
            // (the head of the queue lives in memory, legs_done[b]: wave 0 writes it here and behind a consumed record, every wave reads it behind the
            // barrier of a tick's post; the per-record outputs start as "never")
            if (r.replan && w0 && BMPCK_LANE == 0) {
                r.legs_done[b] = 0;
                for (int k = 0; k < r.legs; k++) {
                    const long long q = (long long)b * r.legs + k;
                    if (r.replan_info) r.replan_info[q] = -1;
                    if (r.leg_fired) r.leg_fired[q] = -1;
                    if (r.leg_why) r.leg_why[q] = 0;
                }
            }
        }
        if (AU) { if (r.audit && BMPCK_LANE == 0) bmpcs::stream_audit_init(r.audit + (long long)b * bmpcs::AUDIT_LEN); }
        if (LG) { if (r.track && BMPCK_LANE == 0) bmpcs::stream_track_init(r.track + (long long)b * bmpcs::TRACK_LEN); }
        int bad = 0;      // (TU) the invalid slots of the stream's row: such a stream runs no tick
        if constexpr (TU) {
            // (every wave reads the row and the kernel arguments itself; lane 0 of wave 0 stores the mask and the row as resolved)
            if (r.tune) {
                const bool out_ = w0 && BMPCK_LANE == 0;
                bad = BMPCK_UNIFORM(bmpc_tune_check(r.tune + (long long)b * bmpctu::LEN, a.o, s, out_ && r.tune_used ? r.tune_used + (long long)b * bmpctu::LEN : nullptr));
                if (out_ && r.tune_info) r.tune_info[b] = bad;
            }
        }
        if constexpr (PL) {
            // (a PL kernel is launched with a table only -- bmpc_rollout_level --, so no line here asks whether there is one.  Every wave reads the row
            // itself; lane 0 of wave 0 stores the mask and starts the record)
            BMPCR_PLANT_ARGS(pl_);
            if (!BMPCR_SE || pl_->plant) {
            int b_ = b; BMPCR_OPAQUE("+s"(b_));
            const int pbad = BMPCK_UNIFORM(bmpc_plant_check(pl_->plant + (long long)b_ * bmpcpl::LEN, nullptr));
            if (w0 && BMPCK_LANE == 0) {
                if (pl_->plant_info) pl_->plant_info[b_] = pbad;
                if (pl_->plant_rec) bmpcs::stream_plant_init(pl_->plant_rec + (long long)b_ * bmpcpl::REC_LEN);
            }
            bad |= pbad;      // (an invalid plant row keeps the stream from running as an invalid settings row does: one word decides)
            }
        }
#if BMPCR_SE
        {
            // (an SE kernel is launched with a sensor table only -- bmpc_rollout_sensor_ok and the entry --, so no line here asks whether there is one.  Every
            // wave reads the row itself; lane 0 of wave 0 stores the mask and starts the record.  An invalid row: as an invalid plant row, state untouched)
            BMPCR_SENSOR_ARGS(se_);
            int b_ = b; BMPCR_SENSOR_IDX(b_);
            const int sbad = BMPCK_UNIFORM(bmpc_sensor_check(se_->sensor + (long long)b_ * bmpcse::LEN, nullptr));
            if (w0 && BMPCK_LANE == 0) {
                if (se_->sensor_info) se_->sensor_info[b_] = sbad;
                if (se_->sensor_rec) bmpcs::stream_sensor_init(se_->sensor_rec + (long long)b_ * bmpcse::REC_LEN);
            }
            bad |= sbad;
#if BMPCR_OB
            // (an OB kernel is launched with an observer table only -- bmpc_rollout_observer_ok and the entry.  Every wave reads the row itself; lane 0 of wave 0
            // stores the mask and starts the record.  An invalid row: as an invalid sensor row, both states untouched)
            BMPCR_OBSERVER_FROM(ob_, se_);
            const int obad = BMPCK_UNIFORM(bmpc_observer_check(ob_->observer + (long long)b_ * bmpcob::LEN, nullptr));
            if (w0 && BMPCK_LANE == 0) {
                if (ob_->observer_info) ob_->observer_info[b_] = obad;
                if (ob_->observer_rec) bmpcs::stream_observer_init(ob_->observer_rec + (long long)b_ * bmpcob::REC_LEN);
            }
            bad |= obad;
#endif
        }
#endif
        if (!TU || !bad) for (; t < r.ticks; t++) {
            // (the lost-plan test of the fused tick: BoundMPC.step() returns five Nones there and the reference node stops)
            if (BMPCK_UNIFORM((int)(ss[bmpcs::SS_ERRCNT] >= (double)a.N))) {
                if (BMPCK_LANE == 0) { a.status[b] = 3; if (a.iters) a.iters[b] = 0; if (a.kkt) a.kkt[b] = 0.0; }
                break;
            }
#if BMPCR_SE
            {
                // The sample: from here to the way back behind the post the robot record is what the sensor hands out, the truth waits in the sensor state.
                // The stream and the tick opaque in vector registers (BMPCR_SENSOR_ARGS).  meas_hist: the record the pack is about to read.
                BMPCR_SENSOR_ARGS(se_);
                int b_ = b, t_ = t;
                BMPCR_SENSOR_IDX(b_); BMPCR_SENSOR_IDX(t_);
                const long long row_ = (long long)t_ * a.B + b_;
#if !BMPCR_OB
                if (w0) bmpcs::stream_sense(se_->sensor + (long long)b_ * bmpcse::LEN, se_->sensor_noise ? se_->sensor_noise + row_ * bmpcs::DIST_LEN : nullptr,
                                            se_->sensor_state + (long long)b_ * bmpcse::ST_LEN, rb, se_->sensor_rec ? se_->sensor_rec + (long long)b_ * bmpcse::REC_LEN : nullptr,
                                            t_, BMPCK_LANE, BMPCK_NL);
#else
                // (the sample followed by the estimate in the same lane-0 section: what the record holds from here to the way back is the observer's estimate,
                // meas_hist the record of it; sample_hist: the raw sample, stored by the lane that made it)
                BMPCR_OBSERVER_FROM(ob_, se_);
                if (w0) bmpcs::stream_observe(a.h, se_->sensor + (long long)b_ * bmpcse::LEN, se_->sensor_noise ? se_->sensor_noise + row_ * bmpcs::DIST_LEN : nullptr,
                                              se_->sensor_state + (long long)b_ * bmpcse::ST_LEN, ob_->observer + (long long)b_ * bmpcob::LEN,
                                              ob_->observer_state + (long long)b_ * bmpcob::ST_LEN, rb, se_->sensor_rec ? se_->sensor_rec + (long long)b_ * bmpcse::REC_LEN : nullptr,
                                              ob_->observer_rec ? ob_->observer_rec + (long long)b_ * bmpcob::REC_LEN : nullptr,
                                              ob_->sample_hist ? ob_->sample_hist + row_ * bmpcs::DIST_LEN : nullptr, t_, BMPCK_LANE, BMPCK_NL);
#endif
                BMPCK_SYNC();      // the pack and the row read the record lane 0 has just stored
                if (se_->meas_hist && w0) { double *mr = se_->meas_hist + row_ * bmpcs::RB_LEN; for (int i = BMPCK_LANE; i < bmpcs::RB_LEN; i += BMPCK_NL) mr[i] = rb[i]; }
            }
#endif
            int N_ = a.N, S_ = a.S;
            BMPCR_OPAQUE("+s"(N_), "+s"(S_));      // (what the stream functions are given)
            if constexpr (!TU) {
                if (w0) bmpcs::stream_pack(N_, S_, path, s.path_stride / bmpcs::PT_LEN, ss, rb, p, x0, dual, (s.flags & 2) ? a.x + (long long)b * nw : nullptr, sh, BMPCK_LANE, BMPCK_NL, s.lvl_c, s.lvl_lo, s.lvl_hi);
            } else {
                SArgs sp = s;      // (what the pack is given: the launch's level rule, or the stream's)
                if (r.tune) { int b_ = b; BMPCR_OPAQUE("+s"(b_)); BMPCR_TUNE_ROW(tr_, b_); bmpc_tune_sargs(tr_, sp); }
                if (w0) bmpcs::stream_pack(N_, S_, path, s.path_stride / bmpcs::PT_LEN, ss, rb, p, x0, dual, (s.flags & 2) ? a.x + (long long)b * nw : nullptr, sh, BMPCK_LANE, BMPCK_NL, sp.lvl_c, sp.lvl_lo, sp.lvl_hi);
            }
            BMPCK_SYNC();
            if (AU) {
                // (the stream and the tick opaque, as for the events: what the audit addresses is computed here and dead before the solve)
                int b_ = b, t_ = t;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_), "+s"(N_), "+s"(S_));
                double *row = r.tube_hist ? r.tube_hist + ((long long)t_ * a.B + b_) * bmpcs::TUBE_LEN : sh;
                if (w0) bmpcs::stream_tube(N_, S_, p, nullptr, row, BMPCK_LANE, BMPCK_NL);      // (no state row: the lost-plan test has just passed)
                if (r.audit && BMPCK_LANE == 0) bmpcs::stream_audit(row, r.audit + (long long)b_ * bmpcs::AUDIT_LEN, t_, r.audit_tol);
                BMPCK_SYNC();      // the solver's reductions reuse the LDS words of the row
            }
            BMPC_WAVE_INIT(W, a, lds, a.scratch + (long long)BMPCK_BLOCK * a.scr_stride, wv); BMPCK_WAVE_HOOK(W);
            if constexpr (TU) { if (r.tune) { int b_ = b; BMPCR_OPAQUE("+s"(b_)); BMPCR_TUNE_ROW(tr_, b_); bmpc_tune_opts(tr_, W.o); } }      // (W.o has just been rebuilt from a.o)
            BMPC_TICK_PROBLEM(pr, a, b, p, x0, dual);
            BMPCR_OPAQUE("+s"(W.N), "+s"(W.S), "+s"(W.h), "+s"(W.G.b), "+s"(pr.p), "+s"(pr.x0), "+s"(pr.x), "+s"(pr.g), "+s"(pr.state));
            const long long t0_ = a.latency_us ? BMPC_NOW() : 0;
            BMPC_NAMESPACE::wave_solve<ZLDS, true, RESTO>(W, pr);
            BMPCK_SYNC();
            if (a.latency_us) busy += BMPC_NOW() - t0_;
            BMPCR_OPAQUE("+s"(N_), "+s"(S_));
            if constexpr (!TU) {
                if (w0) bmpcs::stream_post(N_, S_, a.h, path, s.path_stride / bmpcs::PT_LEN, ss, rb, pr.x, pr.g, a.status[b], traj, s.flags, s.rt_tol, sh, BMPCK_LANE, BMPCK_NL, s.rt_row_cap);
            } else {
                SArgs sq = s;      // (what the post is given: the launch's acceptance words, or the stream's, loaded here, behind the solve)
                if (r.tune) { int b_ = b; BMPCR_OPAQUE("+s"(b_)); BMPCR_TUNE_ROW(tr_, b_); bmpc_tune_sargs(tr_, sq); }
                if (w0) bmpcs::stream_post(N_, S_, a.h, path, s.path_stride / bmpcs::PT_LEN, ss, rb, pr.x, pr.g, a.status[b], traj, s.flags, sq.rt_tol, sh, BMPCK_LANE, BMPCK_NL, sq.rt_row_cap);
            }
            BMPCK_SYNC();      // the history and the next pack read ss, rb, x, traj and the dual state that other lanes have just stored
#if BMPCR_SE
            {
                // The way back: the post has stepped the SAMPLE with the planned jerk; where the sample was not the truth, the truth takes that step here, or
                // comes back as it was where the post did not step.  Every wave reads the two decisions itself -- SAME, which wave 0 stored ahead of the
                // barrier behind the sample and stores next behind the barrier below, and the error count behind the post's barrier --; wave 0 does the work,
                // and the barrier behind it is unconditional.  Ahead of the plant step, the rows and the events: they see the TRUE plant.
                BMPCR_SENSOR_ARGS(se_);
                int b_ = b;
                BMPCR_SENSOR_IDX(b_);
                const double *st_ = se_->sensor_state + (long long)b_ * bmpcse::ST_LEN;
                const int same_ = BMPCK_UNIFORM((int)(st_[bmpcse::ST_SAME] == 1.0)), stepped_ = BMPCK_UNIFORM((int)(ss[bmpcs::SS_ERRCNT] < (double)N_));
                if (!same_) { if (w0) bmpcs::stream_truth(a.h, st_, rb, stepped_ != 0, BMPCK_LANE, BMPCK_NL); }
                BMPCK_SYNC();
            }
#endif
            if constexpr (PL) {
                // The drive between the command the post has just stored and the plant it has just stepped: only where it did step it (every wave reads the
                // error count behind the post's barrier; the pack of the next tick does not write it).  The stream and the tick opaque, as for the events.
                BMPCR_PLANT_ARGS(pl_);
                int b_ = b, t_ = t;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_));
                if ((!BMPCR_SE || pl_->plant) && BMPCK_UNIFORM((int)(ss[bmpcs::SS_ERRCNT] < (double)N_))) {
                    if (w0) bmpcs::stream_plant(a.h, pl_->plant + (long long)b_ * bmpcpl::LEN, pl_->plant_state + (long long)b_ * bmpcpl::ST_LEN, rb,
                                                pl_->plant_rec ? pl_->plant_rec + (long long)b_ * bmpcpl::REC_LEN : nullptr, t_, BMPCK_LANE, BMPCK_NL);
                }
                BMPCK_SYNC();      // the rows, the events and the next pack read the TRUE plant
            }
            const long long row = (long long)t * a.B + b;
            if (r.hist && w0) {
                double *hr = r.hist + row * bmpcs::RH_LEN;
                for (int i = BMPCK_LANE; i < bmpcs::RB_LEN; i += BMPCK_NL) hr[bmpcs::RH_ROBOT + i] = rb[i];
                for (int i = BMPCK_LANE; i < 4; i += BMPCK_NL) hr[bmpcs::RH_NVALID + i] = traj[TRN - 4 + i];
                if (BMPCK_LANE == 0) {
                    hr[bmpcs::RH_PHI] = ss[bmpcs::SS_PHI]; hr[bmpcs::RH_ERRCNT] = ss[bmpcs::SS_ERRCNT]; hr[bmpcs::RH_STATUS] = (double)a.status[b];
                    hr[bmpcs::RH_ITERS] = nan_; hr[bmpcs::RH_KKT] = nan_;
                    if (a.iters) hr[bmpcs::RH_ITERS] = (double)a.iters[b];
                    if (a.kkt) hr[bmpcs::RH_KKT] = a.kkt[b];
                }
            }
            if (r.traj_hist && w0) { double *th = r.traj_hist + row * TRN; for (int i = BMPCK_LANE; i < TRN; i += BMPCK_NL) th[i] = traj[i]; }
            if (LG) {
                // (the stream and the tick opaque, as for the audit: what the log addresses is computed here, behind the solve, and dead before the next one)
                int b_ = b, t_ = t, cap_ = s.path_stride / bmpcs::PT_LEN;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_), "+s"(cap_), "+s"(N_), "+s"(S_));
                // the row: the caller's, or stage 0 alone behind the log's own LDS words
                const int K_ = r.log_hist ? r.log_stages : 1;
                double *lrow = r.log_hist ? r.log_hist + ((long long)t_ * a.B + b_) * (K_ * bmpcs::LOG_STAGE + 4) : sh + bmpcs::LSH_LEN;
                if (w0) bmpcs::stream_log_rows<true>(N_, S_, a.h, path, cap_, ss, p, traj, lrow, K_, sh, BMPCK_LANE, BMPCK_NL);
                // (lane 0 wrote stage 0 and the trailer itself)
                if (r.track && BMPCK_LANE == 0) bmpcs::stream_track(lrow, lrow[K_ * bmpcs::LOG_STAGE], traj[TRN - 3], r.track + (long long)b_ * bmpcs::TRACK_LEN, t_);
                BMPCK_SYNC();      // the events and the next pack reuse the LDS words of the log
            }
            if (EV) {
                // (the stream and the tick opaque: what the events address is computed here, behind the solve, not carried across it)
                int b_ = b, t_ = t, cap_ = s.path_stride / bmpcs::PT_LEN;
                BMPCR_OPAQUE("+s"(b_), "+s"(t_), "+s"(cap_), "+s"(S_));
                if (r.disturb) {
                    if (w0) bmpcs::stream_disturb(rb, r.disturb + ((long long)t_ * a.B + b_) * bmpcs::DIST_LEN, BMPCK_LANE, BMPCK_NL);
                    BMPCK_SYNC();
                }
                if (!QU) {
                    if (r.replan && BMPCK_UNIFORM((int)(r.replan_tick[b_] == t_))) {
                        double *rec = r.replan + (long long)b_ * bmpcs::replan_len(S_, cap_);
                        if (r.update_flags & 2) { if (w0) bmpcs::stream_splice(a.h, S_, cap_, rec, rb, r.update_flags, BMPCK_LANE, BMPCK_NL); BMPCK_SYNC(); }
                        if (w0) bmpcs::stream_update(N_, S_, rec, const_cast<double *>(path), cap_, ss, rb, r.replan_info ? r.replan_info + b_ : nullptr, r.update_flags & 1,
                                             BMPCK_LANE, BMPCK_NL);
                        BMPCK_SYNC();      // the goal test, the lost-plan test and the next pack read what the re-plan stored
                    }
                } else if (r.replan) {
                    // The head record of the stream's queue, legs_done[b], and whether it is due behind this tick: EVERY wave decides for itself, from words
                    // that do not change between the barrier ahead (the post's, the log's or the disturbance's) and the first barrier behind the decision --
                    // the three ss words the stops read, the read-only trigger arrays, and legs_done[b], which wave 0 writes at the start of the stream and
                    // ahead of the last barrier of a consumed record.  Bit 0 of `why`: the record's goal, bit 1: the post of this tick exhausted the plan,
                    // bit 2: at or after its tick.  A word with an unknown bit, or without any condition, is never due: it ends the queue.
                    int L_ = r.legs;
                    BMPCR_OPAQUE("+s"(L_));
                    const int k_ = BMPCK_UNIFORM(r.legs_done[b_]);
                    int why_ = 0;
                    if (k_ < L_) {
                        const long long q_ = (long long)b_ * L_ + k_;
                        const int on_ = r.leg_on[q_], tk_ = r.leg_tick[q_];
                        const double tol_ = r.leg_tol ? r.leg_tol[q_] : r.goal_tol;
                        if (!(on_ & ~(bmpcs::LEG_AT_GOAL | bmpcs::LEG_ON_LOST))) {
                            if ((on_ & bmpcs::LEG_AT_GOAL) && ss[bmpcs::SS_PHIMAX] - ss[bmpcs::SS_PHI] <= tol_) why_ |= bmpcs::LEG_WHY_GOAL;
                            if ((on_ & bmpcs::LEG_ON_LOST) && ss[bmpcs::SS_ERRCNT] >= (double)a.N) why_ |= bmpcs::LEG_WHY_LOST;
                            if (tk_ >= 0 && t_ >= tk_) why_ |= bmpcs::LEG_WHY_TICK;
                        }
                    }
                    why_ = BMPCK_UNIFORM(why_);
                    if (why_) {
                        const long long q_ = (long long)b_ * L_ + k_;
                        double *rec = r.replan + q_ * bmpcs::replan_len(S_, cap_);
                        // (a barrier between the decision, which reads ss, and stream_update, which writes it: the splice's, or one of its own)
                        if (r.update_flags & 2) { if (w0) bmpcs::stream_splice(a.h, S_, cap_, rec, rb, r.update_flags, BMPCK_LANE, BMPCK_NL); }
                        BMPCK_SYNC();
                        // (every wave has read the head ahead of that barrier: it advances here, ahead of the barrier behind stream_update)
                        if (w0 && BMPCK_LANE == 0) {
                            if (r.leg_fired) r.leg_fired[q_] = t_;
                            if (r.leg_why) r.leg_why[q_] = why_;
                            r.legs_done[b_] = k_ + 1;
                        }
                        if (w0) bmpcs::stream_update(N_, S_, rec, const_cast<double *>(path), cap_, ss, rb, r.replan_info ? r.replan_info + q_ : nullptr, r.update_flags & 1,
                                             BMPCK_LANE, BMPCK_NL);
                        BMPCK_SYNC();      // the goal test, the lost-plan test, the next tick's head and the next pack read what the re-plan stored
                    }
                }
            }
            if (BMPCK_UNIFORM((int)(r.goal_tol > 0.0 && ss[bmpcs::SS_PHIMAX] - ss[bmpcs::SS_PHI] <= r.goal_tol))) { t++; break; }
        }
        // t ticks were run; the rows behind them stay without a tick
        for (int u = t; w0 && u < r.ticks; u++) {
            const long long row = (long long)u * a.B + b;
            if (r.hist) for (int i = BMPCK_LANE; i < bmpcs::RH_LEN; i += BMPCK_NL) r.hist[row * bmpcs::RH_LEN + i] = nan_;
            if (r.traj_hist) for (int i = BMPCK_LANE; i < TRN; i += BMPCK_NL) r.traj_hist[row * TRN + i] = nan_;
            if (AU) { if (r.tube_hist) for (int i = BMPCK_LANE; i < bmpcs::TUBE_LEN; i += BMPCK_NL) r.tube_hist[row * bmpcs::TUBE_LEN + i] = nan_; }
            if (LG) {
                const int LR = r.log_stages * bmpcs::LOG_STAGE + 4;
                if (r.log_hist) for (int i = BMPCK_LANE; i < LR; i += BMPCK_NL) r.log_hist[row * LR + i] = nan_;
            }
        }
#if BMPCR_SE
        {
            // (the sensor's rows of the ticks not run, in a loop of their own: the loop above stays the one of the kernels without a sensor)
            BMPCR_SENSOR_ARGS(se_);
            int b_ = b;
            BMPCR_SENSOR_IDX(b_);
            if (se_->meas_hist && w0) {
                for (int u = t; u < r.ticks; u++) {
                    double *mr = se_->meas_hist + ((long long)u * a.B + b_) * bmpcs::RB_LEN;
                    for (int i = BMPCK_LANE; i < bmpcs::RB_LEN; i += BMPCK_NL) mr[i] = nan_;
                }
            }
#if BMPCR_OB
            BMPCR_OBSERVER_FROM(ob_, se_);
            if (ob_->sample_hist && w0) {
                // (ONE loop over the words from row t of the stream to its last row, those of the other streams' rows skipped: as a second nest of two loops
                // here the team kernel with the restoration phase moved a scalar-spill register at the join behind the tick loop, the signature the build's
                // ISA lint refuses.  The last word touched is word DIST_LEN - 1 of row ticks - 1; a stream that ran every tick has n_ <= 0)
                double *sr = ob_->sample_hist + ((long long)t * a.B + b_) * bmpcs::DIST_LEN;
                const long long n_ = (long long)(r.ticks - t - 1) * a.B * bmpcs::DIST_LEN + bmpcs::DIST_LEN;
                for (long long i = BMPCK_LANE; i < n_; i += BMPCK_NL) if (i % ((long long)a.B * bmpcs::DIST_LEN) < bmpcs::DIST_LEN) sr[i] = nan_;
            }
#endif
        }
#endif
        if (BMPCK_LANE == 0) {
            if (r.ticks_run) r.ticks_run[b] = t;
            if (a.latency_us) a.latency_us[b] = (double)busy * 0.01;
        }
        BMPCK_SYNC();      // the next stream's pack reuses the LDS words this stream's last phase read
    }
