// pursuit_crowd_body.inc -- the body of the crowd kernels (pursuit_crowd.hpp), included INSIDE both kernel definitions:
//   pursuit_crowd_kernel<CShape, MODE>        (S::LIVE = false, pending = nullptr): one agent count for the whole batch
//   pursuit_live_crowd_kernel<LCShape, MODE>  (S::LIVE = true): per-env agent counts within the capacity (P, E)
//   pursuit_crowd_to_kernel<S>                (TO = true, MODE = 1): the two-buffer step of madrl_pursuit_step_to (see write_obs)
// In scope: S, MODE, TO, d (CrowdDev), io (CrowdIO), pending (int32 [n_envs][2] or nullptr), obs_prev (TO; nullptr otherwise).
// The environment's rules are pursuit_rules.hpp's.  S::LIVE follows pursuit_generic.inc: a slot that does not exist has position bytes NOT_HERE
// (an evader slot the gone bit too), is never placed in, moved over or taken from the cells, and pursuers >= np get no row and a 0 reward.
    constexpr int P = S::P, E = S::E, A = S::A, GW = S::GW, PAD = S::PAD, GSZ = S::GSZ, NT = S::NT, D = S::D, DV = S::DV, NQ = S::NQ;
    constexpr int R = S::R, OFF = S::OFF, NGW = S::NGW, NTW = S::NTW;
    __shared__ __attribute__((aligned(16))) uint32_t L[S::LDS_DWORDS];
    const int tid0 = threadIdx.x;
    uint32_t *const cell = &L[S::X_CELL];
    float *const s_vtab = reinterpret_cast<float *>(&L[S::X_VTAB]);
    uint32_t *const s_code = &L[S::X_CODE];
    double *const s_rew = reinterpret_cast<double *>(&L[S::X_REW]);
    int32_t *const s_base = reinterpret_cast<int32_t *>(&L[S::X_BASE]);
    int32_t *const s_kpre = reinterpret_cast<int32_t *>(&L[S::X_KPRE]);
    uint32_t *const s_gone = &L[S::X_GONE];
    uint32_t *const s_placed = &L[S::X_PLACED];
    uint32_t *const s_term = &L[S::X_TERM];
    uint32_t *const s_misc = &L[S::X_MISC];
    uint8_t *const s_ax = reinterpret_cast<uint8_t *>(&L[S::X_XY]);
    uint8_t *const s_ay = s_ax + S::A16;

    // ---- once per workgroup: the value table and (flatten) the element codes: channel << 24 | cell offset in the window; channel 3 = the id
    // (compile-time trips, every thread loading from an index clamped to the table's end, all loads before the one wait: "table staging",
    // pursuit_wave.hpp -- the strided loop compiled to one dependent round trip per 64 NW values)
    {
        constexpr int TV = (256 + NT - 1) / NT;
        float vt[TV];
#pragma unroll
        for (int t = 0; t < TV; ++t) {
            const uint32_t k = (uint32_t)tid0 + (uint32_t)(NT * t);
            vt[t] = d.vtab[k < 256u ? k : 255u];
        }
#pragma unroll
        for (int t = 0; t < TV; ++t) {
            const uint32_t k = (uint32_t)tid0 + (uint32_t)(NT * t);
            if (k < 256u) s_vtab[k] = vt[t];
        }
    }
    if constexpr (S::FLATTEN) {
        for (int r = tid0; r < D; r += NT) {
            const int c = r / (R * R), rr = r - c * (R * R), i = rr / R, j = rr - i * R;
            s_code[r] = c == 3 ? (3u << 24) : (((uint32_t)c << 24) | (uint32_t)(i * GW + j));
        }
    }
    int cached_map = -1;   // the map whose bytes the cells hold; the count and credit bytes are zero between envs
    // LIVE: s_misc[5] / [6] = the first pursuer / evader slot that does not exist, found with ds_min where the record is loaded.  They hold
    // (P, E) whenever a load begins: set here and again by the record store of every env, both behind barriers the next load is behind
    if constexpr (S::LIVE) {
        if (tid0 == 0) {
            s_misc[5] = (uint32_t)P;
            s_misc[6] = (uint32_t)E;
        }
    }

    for (int64_t env = blockIdx.x; env < d.n_envs; env += gridDim.x) {
        if (MODE == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // block-uniform
        // (a fresh copy per env: what is derived from the thread index -- LDS addresses, lane predicates -- is then computed where it is
        // used instead of being held in registers across the env loop, which the 128 registers of a 16-wavefront workgroup cannot afford)
        const int tid = fresh(tid0);
        uint8_t *rec = d.state + env * (int64_t)S::REC_BYTES;
        group_sync();  // the previous env's LDS traffic is finished
        // ------------------------------------------------------------ load state record
        if (tid < 4) s_misc[tid] = reinterpret_cast<const uint32_t *>(rec)[tid];
        if (tid == 4) s_misc[4] = 0;
        for (int a = tid; a < A; a += NT) {
            const uint32_t xy = reinterpret_cast<const uint16_t *>(rec + HDR_BYTES)[a];
            s_ax[a] = (uint8_t)(xy & 0xFF);
            s_ay[a] = (uint8_t)(xy >> 8);
            if constexpr (S::LIVE) {
                if ((xy & 0xFFu) == NOT_HERE) atomicMin(&s_misc[a < P ? 5 : 6], (uint32_t)(a < P ? a : a - P));
            }
        }
        for (int w = tid; w < NGW; w += NT) {
            const uint32_t g = reinterpret_cast<const uint32_t *>(rec + S::OFF_GONE)[w];
            s_gone[w] = g;
            s_placed[w] = ~g;   // step mode: the evaders the pre-move pass counts
        }
        for (int w = tid; w < NTW; w += NT) s_term[w] = reinterpret_cast<const uint32_t *>(rec + S::OFF_TERM)[w];
        const bool ch3_zero = !S::FLATTEN && d.ch3[env] == 0u;
        group_sync();
        uint32_t tick = s_misc[0];
        int32_t tstep = (int32_t)s_misc[1];
        int32_t map_id = (int32_t)s_misc[2];
        const uint32_t gid = d.gid_base + (uint32_t)env;
        bool do_reset = (MODE == 0);
        uint32_t done_bits = 0;
        int np = P, ne = E;  // live pursuers / evader slots (LIVE; the capacity otherwise)
        if constexpr (S::LIVE) {
            np = __builtin_amdgcn_readfirstlane((int)s_misc[5]);
            ne = __builtin_amdgcn_readfirstlane((int)s_misc[6]);
        }

        // the cells take the map's bytes (count and credit bytes: zero).  Only called while no agent is placed.
        auto load_map = [&](int m) {
            if (cached_map == m) return;
            const uint32_t *mt = reinterpret_cast<const uint32_t *>(d.maps + (int64_t)m * d.map_stride);
            // batches of at most 8 compile-time trips: the batch's loads (clamped to the map's last word), one wait, its LDS writes
            constexpr int MAPW = GSZ / 4, TM = (MAPW + NT - 1) / NT;
#pragma unroll
            for (int t0 = 0; t0 < TM; t0 += 8) {
                uint32_t mw[8];
#pragma unroll
                for (int t = t0; t < (t0 + 8 < TM ? t0 + 8 : TM); ++t) {
                    const uint32_t k = (uint32_t)tid + (uint32_t)(NT * t);
                    mw[t - t0] = mt[k < (uint32_t)MAPW ? k : (uint32_t)MAPW - 1u];
                }
#pragma unroll
                for (int t = t0; t < (t0 + 8 < TM ? t0 + 8 : TM); ++t) {
                    const uint32_t k = (uint32_t)tid + (uint32_t)(NT * t), w = mw[t - t0];
                    if (k < (uint32_t)MAPW) reinterpret_cast<uint4 *>(cell)[k] = make_uint4(w & 0xFFu, (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, w >> 24);
                }
            }
            cached_map = m;
        };

        // -------------------------------------------------------------- observations (:418-461)
        // TO, src != nullptr: the two-buffer pass -- every float4 of the env's P rows leaves as one whole non-temporal store to io.obs; the
        // elements the in-place pass does not store come from the same float4 of `src` (loaded only then; channel 3 of an (R, R, 4) row
        // only while the env's word says "not known zero"), and the rows of pursuers that do not exist are copied whole.  src == nullptr:
        // the in-place pass on io.obs (the second pass of a fused auto-reset, over the step pass's rows).
        auto write_obs = [&]([[maybe_unused]] const float *src) {
            // (the env's rows through a wave-uniform base and 32-bit offsets: P * D floats are far below 4 GB)
            typedef __attribute__((address_space(1))) float gfloat;
            typedef __attribute__((address_space(1))) v4f gv4f;
            gfloat *const orow = uniform_ptr(io.obs + env * (int64_t)P * D);
            if constexpr (TO) {
                if (src != nullptr) {
                    typedef const __attribute__((address_space(1))) v4f cgv4f;
                    cgv4f *const prow = reinterpret_cast<cgv4f *>(uniform_ptr(src + env * (int64_t)P * D));
                    int p = tid / DV, f = tid - p * DV;
                    constexpr int dp = NT / DV, df = NT - dp * DV;
                    [[maybe_unused]] const double n_id = (double)np;
                    for (uint32_t q = (uint32_t)tid; q < (uint32_t)NQ; q += (uint32_t)NT) {
                        gv4f *const o = reinterpret_cast<gv4f *>(orow + 4u * q);
                        v4f v;
                        if (S::LIVE && p >= np) {
                            v = prow[q];
                        } else {
                            const int base = s_base[p];
                            float idv;
                            if constexpr (S::LIVE) idv = (float)((double)p / n_id);
                            else idv = (float)((double)p / (double)P);  // :440-445
                            if constexpr (S::FLATTEN) {
                                const uint4 cd = reinterpret_cast<const uint4 *>(s_code)[f];
                                const uint32_t code[4] = {cd.x, cd.y, cd.z, cd.w};
                                float val[4];
                                bool keep[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const uint32_t ch = code[k] >> 24;
                                    if (ch == 3u) {
                                        val[k] = idv;
                                        keep[k] = true;
                                    } else {
                                        const uint32_t c = cell[base + (int)(code[k] & 0xFFFFFFu)];
                                        val[k] = s_vtab[(c >> (8u * ch)) & 0xFFu];
                                        keep[k] = ch == 0u || (c & 0xFFu) != PAD_MAP;
                                    }
                                }
                                v = v4f{val[0], val[1], val[2], val[3]};
                                if (!(keep[0] & keep[1] & keep[2] & keep[3])) {
                                    const v4f old = prow[q];
                                    if (!keep[0]) v.x = old.x;
                                    if (!keep[1]) v.y = old.y;
                                    if (!keep[2]) v.z = old.z;
                                    if (!keep[3]) v.w = old.w;
                                }
                            } else {
                                const int i = f / R, j = f - i * R;
                                const uint32_t c = cell[base + i * GW + j];
                                const bool outside = (c & 0xFFu) == PAD_MAP;
                                v = v4f{s_vtab[c & 0xFFu], s_vtab[(c >> 8) & 0xFFu], s_vtab[(c >> 16) & 0xFFu], 0.0f};
                                if (!outside && f == S::CENTRE) {
                                    v.w = idv;
                                } else if (outside || !ch3_zero) {
                                    const v4f old = prow[q];
                                    if (outside) { v.y = old.y; v.z = old.z; }
                                    if (!ch3_zero) v.w = old.w;
                                }
                            }
                        }
                        __builtin_nontemporal_store(v, o);
                        f += df; p += dp;
                        if (f >= DV) { f -= DV; ++p; }
                    }
                    return;
                }
            }
            int p = tid / DV, f = tid - p * DV;
            constexpr int dp = NT / DV, df = NT - dp * DV;
            // LIVE: np * DV slots -- rows of pursuers that do not exist keep their contents.  The loop counts its iterations, so that the
            // run-time bound unrolls as the constant one does: two slots without a test between them, and a remainder
            uint32_t n_it = 0;
            if constexpr (S::LIVE) n_it = (uint32_t)(np * DV) > (uint32_t)tid ? ((uint32_t)(np * DV) - (uint32_t)tid + (uint32_t)(NT - 1)) / (uint32_t)NT : 0u;
            [[maybe_unused]] const double n_id = (double)np;
#pragma unroll 2
            for (uint32_t q = (uint32_t)tid, it = 0; S::LIVE ? it < n_it : q < (uint32_t)NQ; q += (uint32_t)NT, ++it) {
                const int base = s_base[p];
                gfloat *const o = orow + 4u * q;
                if constexpr (S::FLATTEN) {
                    const uint4 cd = reinterpret_cast<const uint4 *>(s_code)[f];
                    const uint32_t code[4] = {cd.x, cd.y, cd.z, cd.w};
                    float val[4];
                    bool keep[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t ch = code[k] >> 24;
                        if (ch == 3u) {
                            if constexpr (S::LIVE) val[k] = (float)((double)p / n_id);
                            else val[k] = (float)((double)p / (double)P);  // :440-445
                            keep[k] = true;
                        } else {
                            const uint32_t c = cell[base + (int)(code[k] & 0xFFFFFFu)];
                            val[k] = s_vtab[(c >> (8u * ch)) & 0xFFu];
                            keep[k] = ch == 0u || (c & 0xFFu) != PAD_MAP;  // count cells outside the map keep their old contents
                        }
                    }
                    if (keep[0] & keep[1] & keep[2] & keep[3]) {
                        const v4f v = {val[0], val[1], val[2], val[3]};
                        __builtin_nontemporal_store(v, reinterpret_cast<gv4f *>(o));
                    } else {
                        if (keep[0]) o[0] = val[0];
                        if (keep[1]) o[1] = val[1];
                        if (keep[2]) o[2] = val[2];
                        if (keep[3]) o[3] = val[3];
                    }
                } else {
                    const int i = f / R, j = f - i * R;
                    const uint32_t c = cell[base + i * GW + j];
                    const float v0 = s_vtab[c & 0xFFu];
                    if ((c & 0xFFu) == PAD_MAP) {
                        o[0] = v0;   // outside the map: the fill value in channel 0, the counts keep their old contents
                    } else {
                        const float v1 = s_vtab[(c >> 8) & 0xFFu], v2 = s_vtab[(c >> 16) & 0xFFu];
                        if (f == S::CENTRE) {
                            float idv;
                            if constexpr (S::LIVE) idv = (float)((double)p / n_id);
                            else idv = (float)((double)p / (double)P);  // :440-445
                            const v4f v = {v0, v1, v2, idv};
                            __builtin_nontemporal_store(v, reinterpret_cast<gv4f *>(o));
                        } else if (ch3_zero) {
                            const v4f v = {v0, v1, v2, 0.0f};
                            __builtin_nontemporal_store(v, reinterpret_cast<gv4f *>(o));
                        } else {   // channel 3 off the centre is never written (:440-441)
                            o[0] = v0;
                            o[1] = v1;
                            o[2] = v2;
                        }
                    }
                }
                f += df; p += dp;
                if (f >= DV) { f -= DV; ++p; }
            }
        };

        // the placed agents leave the cells: counts first, then (behind a barrier: a count that left its byte may have carried into the
        // credit bit) the credit of the evaders caught in this step
        auto undo = [&]() {
            group_sync();  // the row pass has read the cells
            for (int a = tid; a < A; a += NT) {
                if constexpr (S::LIVE) {
                    if (a < P ? a >= np : a - P >= ne) continue;  // a slot that does not exist was never placed
                }
                const int idx = (s_ax[a] + PAD) * GW + s_ay[a] + PAD;
                if (a < P) atomicSub(&cell[idx], 1u << 8);
                else if ((s_placed[(a - P) >> 5] >> ((a - P) & 31)) & 1u) atomicSub(&cell[idx], 1u << 16);
            }
            group_sync();
            for (int i = tid; i < E; i += NT) {
                if (!((s_placed[i >> 5] & s_gone[i >> 5]) >> (i & 31) & 1u)) continue;
                const int c0 = (s_ax[P + i] + PAD) * GW + s_ay[P + i] + PAD;
                atomicAnd(&cell[c0], 0x00FFFFFFu);
                atomicAnd(&cell[c0 - GW], 0x00FFFFFFu);
                atomicAnd(&cell[c0 + GW], 0x00FFFFFFu);
                atomicAnd(&cell[c0 + 1], 0x00FFFFFFu);
                atomicAnd(&cell[c0 - 1], 0x00FFFFFFu);
            }
        };

        if constexpr (MODE == 1) {
            load_map(map_id);
            group_sync();
            // -------------------------------------------------------- pre-move evader counts (:364-365)
            for (int i = tid; i < E; i += NT) {
                if (!((s_gone[i >> 5] >> (i & 31)) & 1u)) cell_add(cell, (s_ax[P + i] + PAD) * GW + s_ay[P + i] + PAD, 16u, &s_misc[3]);
            }
            group_sync();
            // proximity reward on the PRE-move state, np.clip keeps border pursuers on their own cell (:374-380)
            for (int p = tid; p < (S::LIVE ? np : P); p += NT) {
                const int x = s_ax[p], y = s_ay[p];
                const int xm = max(x - 1, 0), xp = min(x + 1, S::XS - 1);
                const int ym = max(y - 1, 0), yp = min(y + 1, S::YS - 1);
                s_kpre[p] = (int)((cell[(xm + PAD) * GW + y + PAD] >> 16) & 0xFFu) + (int)((cell[(xp + PAD) * GW + y + PAD] >> 16) & 0xFFu) +
                            (int)((cell[(x + PAD) * GW + yp + PAD] >> 16) & 0xFFu) + (int)((cell[(x + PAD) * GW + ym + PAD] >> 16) & 0xFFu);
            }
            group_sync();
            // -------------------------------------------------------- moves (:229-241)
            for (int a = tid; a < A; a += NT) {
                const bool is_p = a < P;
                const int i = a - P;
                if (!is_p && ((s_gone[i >> 5] >> (i & 31)) & 1u)) continue;
                if constexpr (S::LIVE) {
                    if (is_p && a >= np) continue;  // a pursuer slot this episode does not have
                }
                int x = s_ax[a], y = s_ay[a];
                int act;
                if (is_p) {
                    act = io.actions[env * P + a];
                } else {
                    atomicSub(&cell[(x + PAD) * GW + y + PAD], 1u << 16);  // undo the pre-move count
                    int k = 0;  // index in the evader LAYER = alive evaders in slots below i
                    for (int w = 0; w < (i >> 5); ++w) k += 32 - __popc(s_gone[w]);
                    k += (i & 31) - __popc(s_gone[i >> 5] & ((1u << (i & 31)) - 1u));
                    if (io.inj_eact != nullptr) {
                        act = io.inj_eact[env * E + k];
                    } else act = pr::evader_action(gid, tick, (uint32_t)k, d.k0, d.k1);
                }
                // DiscreteAgent.step, DiscreteAgent.py:69-97
                const bool term = (s_term[a >> 5] >> (a & 31)) & 1u;
                if (!term) {
                    if ((cell[(x + PAD) * GW + y + PAD] & 0xFFu) == 1u) {
                        atomicOr(&s_term[a >> 5], 1u << (a & 31));  // standing in a building
                    } else {
                        int nx = x, ny = y;
                        if (act == 0) nx = x - 1;
                        else if (act == 1) nx = x + 1;
                        else if (act == 2) ny = y + 1;
                        else if (act == 3) ny = y - 1;
                        if ((cell[(nx + PAD) * GW + ny + PAD] & 0xFFu) == 0u) {  // 0 = free, 1 = building, 0xFE = outside the map
                            x = nx;
                            y = ny;
                        }
                    }
                }
                s_ax[a] = (uint8_t)x;
                s_ay[a] = (uint8_t)y;
                if (is_p) s_base[a] = (x - OFF + PAD) * GW + (y - OFF + PAD);
                cell_add(cell, (x + PAD) * GW + y + PAD, is_p ? 8u : 16u, &s_misc[3]);  // :244-246
            }
            group_sync();
            // -------------------------------------------------------- catch resolution (:463-521)
            const uint8_t *need_tab = d.maps + (int64_t)map_id * d.map_stride + GSZ;
            for (int i = tid; i < E; i += NT) {
                if ((s_gone[i >> 5] >> (i & 31)) & 1u) continue;
                const int x = s_ax[P + i], y = s_ay[P + i];
                const int c0 = (x + PAD) * GW + y + PAD;
                bool caught;
                // a neighbour holds pursuers: its count byte is 1 .. 254 (cells outside the map never hold any)
                auto hit = [&](int c) { return (uint8_t)(((cell[c] >> 8) & 0xFFu) - 1u) < 0xFEu; };
                if (d.surround) {
                    const bool h0 = hit(c0 - GW), h1 = hit(c0 + GW), h2 = hit(c0 + 1), h3 = hit(c0 - 1);  // neighbour order of surround_mask (:150)
                    const int cnt = (int)h0 + (int)h1 + (int)h2 + (int)h3;
                    caught = (cnt == (int)need_tab[x * S::YS + y]);  // need_to_surround :523-540
                    if (caught) {  // pursuers standing on a matched neighbour get credit (:489-495)
                        if (h0) atomicOr(&cell[c0 - GW], 1u << 24);
                        if (h1) atomicOr(&cell[c0 + GW], 1u << 24);
                        if (h2) atomicOr(&cell[c0 + 1], 1u << 24);
                        if (h3) atomicOr(&cell[c0 - 1], 1u << 24);
                    }
                } else {
                    caught = (int)((cell[c0] >> 8) & 0xFFu) >= d.n_catch;  // :498
                    if (caught) atomicOr(&cell[c0], 1u << 24);             // :503-506
                }
                if (caught) {
                    atomicOr(&s_gone[i >> 5], 1u << (i & 31));
                    atomicAdd(&s_misc[4], 1u);
                }
            }
            group_sync();
            // -------------------------------------------------------- rewards (:254-262)
            int n_alive = E;
            for (int w = 0; w < NGW; ++w) n_alive -= __popc(s_gone[w]);
            const double catchr = d.catchr_env ? d.catchr_env[env] : d.catchr;
            for (int p = tid; p < P; p += NT) {
                if constexpr (S::LIVE) {
                    if (p >= np) {  // no such pursuer: reward 0
                        io.rew[env * P + p] = 0.0f;
                        continue;
                    }
                }
                const uint32_t sur = (cell[(s_ax[p] + PAD) * GW + s_ay[p] + PAD] >> 24) & 1u;
                const double r = pr::pursuer_reward(catchr, s_kpre[p], d.term_pursuit, sur, d.urgency);
                if (d.reward_global) s_rew[p] = r;
                else io.rew[env * P + p] = (float)r;
            }
            if (d.reward_global) {
                group_sync();
                if constexpr (S::LIVE) {
                    if (tid < np) {
                        const double m = np_sum_n(s_rew, np) / (double)np;
                        for (int p = tid; p < np; p += NT) io.rew[env * P + p] = (float)m;
                    }
                } else if (tid < P) {
                    const double m = np_sum<P>(s_rew) / (double)P;
                    for (int p = tid; p < P; p += NT) io.rew[env * P + p] = (float)m;
                }
            }
            tick += 1;
            tstep += 1;
            done_bits = pr::done_bits(n_alive == 0, d.max_steps, tstep);
            const uint32_t overflow = s_misc[3] ? 0x80u : 0u;                // a cell's count left the byte range: results void
            if (tid == 0) {
                io.done[env] = (uint8_t)(done_bits | overflow);
                io.removed[env] = (int32_t)s_misc[4];
                d.flags[env] = done_flag_word(done_bits | overflow);
            }
            do_reset = d.auto_reset && done_bits != 0;
        }
        // a step: the rows of the step; with auto-reset the reference sequence is step() then reset(), both write the persistent observation
        // buffer, and cells the second write skips keep the first one's values.  A reset launch: the reset, then its rows.
        for (int pass = MODE == 0 ? 1 : 0;; ++pass) {
            if (pass == 1) {
                // ---------------------------------------------------------- reset (:173-207)
                group_sync();
                if (tid == 0) s_misc[3] = 0u;                         // a new episode: the overflow mark goes
                for (int w = tid; w < NGW; w += NT) s_gone[w] = 0u;   // :175-176
                for (int w = tid; w < NTW; w += NT) s_term[w] = 0u;   // fresh agents
                if (io.inj_map != nullptr && MODE == 0) map_id = io.inj_map[env];
                else if (d.sample_maps) map_id = pr::reset_map_id(gid, tick, d.k0, d.k1, d.n_maps);
                load_map(map_id);
                const pr::Window win = pr::reset_window(gid, tick, d.k0, d.k1, d.cw_env ? d.cw_env[env] : d.cw, S::XS, S::YS);
                const bool inj = io.inj_pos != nullptr && MODE == 0;   // (an injected position with x < 0 marks an evader slot that is not created)
                int n_create = E;
                if constexpr (S::LIVE) {  // the pending counts take effect
                    const pr::Counts live = pr::clamp_pending(uniform_ptr(pending + 2 * env)[0], uniform_ptr(pending + 2 * env)[1], P, E);
                    np = live.np, ne = n_create = live.ne;
                }
                if (d.max_opponents > 0 && !inj) n_create = pr::reset_n_create(gid, tick, d.k0, d.k1, d.max_opponents, S::LIVE ? ne : E);
                group_sync();
                for (int a = tid; a < A; a += NT) {  // create_agents, agent_utils.py:12-28
                    int x = 0, y = 0;
                    if constexpr (S::LIVE) {
                        if (a < P ? a >= np : a - P >= ne) {  // a slot this episode does not have
                            if (a >= P) atomicOr(&s_gone[(a - P) >> 5], 1u << ((a - P) & 31));
                            s_ax[a] = (uint8_t)NOT_HERE;
                            s_ay[a] = (uint8_t)NOT_HERE;
                            continue;
                        }
                    }
                    if (a >= P && (a - P >= n_create || (inj && io.inj_pos[(env * A + a) * 2] < 0))) {
                        atomicOr(&s_gone[(a - P) >> 5], 1u << ((a - P) & 31));
                        s_ax[a] = 0;
                        s_ay[a] = 0;
                        continue;
                    }
                    if (inj) {
                        x = io.inj_pos[(env * A + a) * 2];
                        y = io.inj_pos[(env * A + a) * 2 + 1];
                        // (an injected position is the caller's word, as in the generic kernel; only the LDS index is kept inside the grid)
                        x = min(max(x, 0), S::XS - 1);
                        y = min(max(y, 0), S::YS - 1);
                    } else {
                        for (uint32_t att = 0; att < 1024u; ++att) {   // bounded, like the oracle's
                            const uint32_t aidx = S::LIVE ? pr::live_agent_index(a, P, np) : (uint32_t)a;
                            const pr::Cell c = pr::reset_cell(gid, tick, aidx, att, d.k0, d.k1, win);
                            x = c.x, y = c.y;
                            if ((cell[(x + PAD) * GW + y + PAD] & 0xFFu) != 1u) break;
                        }
                    }
                    s_ax[a] = (uint8_t)x;
                    s_ay[a] = (uint8_t)y;
                    if (a < P) s_base[a] = (x - OFF + PAD) * GW + (y - OFF + PAD);
                    cell_add(cell, (x + PAD) * GW + y + PAD, a < P ? 8u : 16u, &s_misc[3]);  // :201-203
                }
                tick += 1;
                tstep = 0;
                group_sync();
                for (int w = tid; w < NGW; w += NT) s_placed[w] = ~s_gone[w];
                group_sync();
            }
            write_obs(pass == 0 ? obs_prev : nullptr);   // (a step: the barrier after the catches published everything the rows read)
            if (pass == 1 || !do_reset) break;
            undo();
        }
        // -------------------------------------------------------------- store state record
        for (int a = tid; a < A; a += NT)
            reinterpret_cast<uint16_t *>(rec + HDR_BYTES)[a] = (uint16_t)(s_ax[a] | (s_ay[a] << 8));
        for (int w = tid; w < NGW; w += NT) reinterpret_cast<uint32_t *>(rec + S::OFF_GONE)[w] = s_gone[w];
        for (int w = tid; w < NTW; w += NT) reinterpret_cast<uint32_t *>(rec + S::OFF_TERM)[w] = s_term[w];
        if (tid == 0) {
            uint32_t *h = reinterpret_cast<uint32_t *>(rec);
            h[0] = tick;
            h[1] = (uint32_t)tstep;
            h[2] = (uint32_t)map_id;
            h[3] = s_misc[3];   // sticky count-overflow mark of the episode
            if constexpr (S::LIVE) {  // (every thread read them behind the load's barrier; the next load is behind undo()'s)
                s_misc[5] = (uint32_t)P;
                s_misc[6] = (uint32_t)E;
            }
        }
        undo();
    }
