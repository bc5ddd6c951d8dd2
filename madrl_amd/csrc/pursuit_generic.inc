// pursuit_generic.inc -- the body of the generic PursuitEvade kernels (pursuit.hip), included INSIDE both kernel definitions:
//   pursuit_kernel<NT>       (LIVE = false, pending = nullptr): one agent count for the whole batch
//   pursuit_live_kernel<NT>  (LIVE = true): per-env agent counts
//   pursuit_to_kernel<NT, LIVE>  (TO = true): the two-buffer step of madrl_pursuit_step_to -- the step's rows go to io.obs, the cells an
//                            in-place step leaves alone come from obs_prev (see write_obs)
//   pursuit_to_f16_kernel<NT, LIVE>  (TO and H16 = true): the same over binary16 buffers (madrl_pursuit_step_to_f16) -- io.obs and obs_prev
//                            point at 2-byte elements, a stored value is the round-to-nearest-even half of the float32 one, a kept
//                            element is its 16 bits copied
// It is included rather than called because a __device__ function between the kernel and its body changes the code the compiler
// emits for pursuit_kernel<NT> (its passes see the body on its own before inlining it).  The environment's rules are pursuit_rules.hpp's.
// In scope: NT, LIVE, TO, H16, d (PursuitDev), io (PursuitIO), mode, pending (int32 [n_envs][2] or nullptr), obs_prev (TO; nullptr otherwise).
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int nthr = blockDim.x;

    // ---- LDS carve (all offsets multiples of 16)
    float *s_vtab = reinterpret_cast<float *>(smem);                   // 256 floats
    uint8_t *g_map = smem + 1024;                                      // 3 layers, contiguous:
    uint8_t *g_pc = g_map + d.GSZ;                                     //   map | pursuers | evaders
    uint8_t *g_ec = g_pc + d.GSZ;
    uint8_t *g_cr = g_ec + d.GSZ;                                      // credit layer (purs_sur)
    const int A16 = (d.A + 15) & ~15;
    uint8_t *s_ax = g_cr + d.GSZ;
    uint8_t *s_ay = s_ax + A16;
    uint32_t *s_gone = reinterpret_cast<uint32_t *>(s_ay + A16);       // ngw words
    uint32_t *s_term = s_gone + ((d.ngw + 3) & ~3);                    // ntw words
    uint32_t *s_misc = s_term + ((d.ntw + 3) & ~3);                    // [0..3] header, [4] removed
    int32_t *s_kpre = reinterpret_cast<int32_t *>(s_misc + 8);         // P ints (pre-move counts)
    double *s_rew = reinterpret_cast<double *>(s_kpre + ((d.P + 3) & ~3));  // P doubles
    uint32_t *s_code = reinterpret_cast<uint32_t *>(s_rew + ((d.P + 1) & ~1));  // D slot codes (float4 observation path)
    // observers: whose windows the P observation rows show.  train_pursuit: pursuer p.  Evader control (:204-207, :251 with
    // agent_layer = evader_layer): row k = the k-th remaining evader among slots 0..P-1 (collect_obs :418-428 walks
    // range(n_agents()) = range(n_pursuers) over evaders_gone and indexes the compacted layer); s_misc[5] = number of rows
    uint8_t *s_ox = reinterpret_cast<uint8_t *>(s_code + ((d.D + 3) & ~3));
    uint8_t *s_oy = s_ox + ((d.P + 15) & ~15);

    // ---- once per workgroup: value table and this thread's observation slot codes
    for (int k = tid; k < 256; k += nthr) s_vtab[k] = d.vtab[k];
    const bool vec4 = (d.D & 3) == 0;  // rows are whole float4s (always for odd obs_range)
    if (vec4) for (int k = tid; k < d.D; k += nthr) s_code[k] = d.codes[k];
    uint32_t code[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int r = tid + t * nthr;
        code[t] = (r < d.D) ? d.codes[r] : (K_SKIP << 24);
    }
    const int GW = d.GW, pad = d.pad, GSZ = d.GSZ;
    const int obs_off = (d.R - 1) / 2;  // pursuit_evade.py:65
    const int gsz_words = GSZ >> 2;
    int cached_map = -1;

    for (int64_t env = blockIdx.x; env < d.n_envs; env += gridDim.x) {
        if (mode == 0 && io.mask != nullptr && io.mask[env] == 0) continue;  // block-uniform
        uint8_t *rec = d.state + env * (int64_t)d.rec_bytes;
        __syncthreads();  // previous env's LDS reads are finished
        // ------------------------------------------------------------ load state record
        if (tid < 4) s_misc[tid] = reinterpret_cast<const uint32_t *>(rec)[tid];
        if (tid == 4) s_misc[4] = 0;
        for (int a = tid; a < d.A; a += nthr) {
            const uint32_t xy = reinterpret_cast<const uint16_t *>(rec + HDR_BYTES)[a];
            s_ax[a] = (uint8_t)(xy & 0xFF);
            s_ay[a] = (uint8_t)(xy >> 8);
        }
        for (int w = tid; w < d.ngw; w += nthr)
            s_gone[w] = reinterpret_cast<const uint32_t *>(rec + d.off_gone)[w];
        for (int w = tid; w < d.ntw; w += nthr)
            s_term[w] = reinterpret_cast<const uint32_t *>(rec + d.off_term)[w];
        __syncthreads();
        uint32_t tick = s_misc[0];
        int32_t tstep = (int32_t)s_misc[1];
        int32_t map_id = (int32_t)s_misc[2];
        const uint32_t gid = d.gid_base + (uint32_t)env;
        bool do_reset = (mode == 0);
        uint32_t done_bits = 0;
        int np = d.P, ne = d.E;  // live pursuers / evader slots (LIVE; the capacity otherwise)
        if constexpr (LIVE) {
            np = 0;
            while (np < d.P && s_ax[np] != NOT_HERE) ++np;
            ne = 0;
            while (ne < d.E && s_ax[d.P + ne] != NOT_HERE) ++ne;
        }

        // -------------------------------------------------------------- observations (:418-461)
        // Element r of pursuer p's row: code[] says which padded-grid byte (relative to the
        // window origin) feeds it.  Stores are lane-contiguous dwords; cells of the count
        // layers outside the map read 0xFF and are NOT stored (reference leaves them stale).
        // TO, src != nullptr: the two-buffer pass.  Every element of the env's rows is stored to io.obs; an element the in-place pass
        // would not store (count cells outside the map, skipped cells, rows of absent observers) is loaded from the same place of `src`,
        // and only the float4s that hold such an element are loaded.  src == nullptr is the in-place pass on io.obs: the second pass of a
        // fused auto-reset, which sees the first pass's values there.
        auto write_obs = [&]([[maybe_unused]] const float *src) {
#if defined(MADRL_ABLATE) && (MADRL_ABLATE & 8)
            if (d.n_envs >= 0) return;
#endif
            float *orow = io.obs + env * (int64_t)d.P * d.D;
            [[maybe_unused]] const float *prow = nullptr;
            if constexpr (TO) prow = src ? src + env * (int64_t)d.P * d.D : nullptr;
            int n_rows = LIVE ? np : d.P;
            if (!d.train_pursuit) {  // observers = the remaining evaders of slots 0..P-1, in slot order
                __syncthreads();
                if (tid == 0) {
                    int k = 0;
                    for (int i = 0; i < d.P && i < d.E; ++i)
                        if (!((s_gone[i >> 5] >> (i & 31)) & 1u)) { s_ox[k] = s_ax[d.P + i]; s_oy[k] = s_ay[d.P + i]; ++k; }
                    s_misc[5] = (uint32_t)k;
                }
                __syncthreads();
                n_rows = (int)s_misc[5];
            }
            const uint8_t *obx = d.train_pursuit ? s_ax : s_ox, *oby = d.train_pursuit ? s_ay : s_oy;
            if (vec4) {
                // float4 path (same scheme as the wave kernel): the P*D/4 float4 slots of the env are spread over the threads;
                // a slot without stale cells is ONE non-temporal 16-byte store, a slot with stale cells falls back to masked
                // dword stores (plain, merged in L2).  One float4 instruction touches each 64-byte chunk once, where the
                // per-pursuer dword rows re-touch the row tails (DESIGN.md 4.3, scripts/ubench/vmem_issue.hip).
                typedef float v4f __attribute__((ext_vector_type(4)));
                const int DV = d.D >> 2, NQ = d.P * DV;
                int p = tid / DV, f = tid - p * DV;
                const int dp = nthr / DV, df = nthr - dp * DV;
                if constexpr (H16) {
                    // binary16 buffers: the slot is the same four elements, 8 bytes.  Two buffers: one whole non-temporal store per slot, the
                    // kept halves from the previous buffer's word.  In place (the second pass of a fused auto-reset): a slot without kept
                    // elements is one store, any other slot plain 2-byte stores of the elements that are written.
                    typedef uint16_t v4h __attribute__((ext_vector_type(4)));
                    uint16_t *orow16 = reinterpret_cast<uint16_t *>(io.obs) + env * (int64_t)d.P * d.D;
                    const uint16_t *prow16 = src ? reinterpret_cast<const uint16_t *>(src) + env * (int64_t)d.P * d.D : nullptr;
                    for (int q = tid; q < NQ; q += nthr) {
                        uint16_t *o = orow16 + 4 * (int64_t)q;
                        if (p >= n_rows) {  // rows of absent observers: copied whole as 16-bit data (in place: they keep their contents)
                            if (prow16 == nullptr) break;
                            __builtin_nontemporal_store(*reinterpret_cast<const v4h *>(prow16 + 4 * (int64_t)q), reinterpret_cast<v4h *>(o));
                        } else {
                            const int base = (obx[p] - obs_off + pad) * GW + (oby[p] - obs_off + pad);
                            v4h v;
                            bool store[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const uint32_t c = s_code[4 * f + k];
                                const uint32_t kind = c >> 24;
                                store[k] = true;
                                float val = 0.0f;
                                if (kind == K_GRID) {
                                    const uint32_t g = g_map[base + (int)(c & 0xFFFFFFu)];
                                    store[k] = g != PAD_CNT;
                                    val = s_vtab[g];
                                } else if (kind == K_ID) {
                                    val = (float)((double)p / (double)(LIVE ? np : d.P));
                                } else if (kind == K_FILL) {
                                    val = d.fill32;
                                } else {
                                    store[k] = false;
                                }
                                v[k] = half_bits(val);
                            }
                            const bool whole = store[0] & store[1] & store[2] & store[3];
                            if (prow16 != nullptr) {
                                if (!whole) {
                                    const v4h old = *reinterpret_cast<const v4h *>(prow16 + 4 * (int64_t)q);
#pragma unroll
                                    for (int k = 0; k < 4; ++k)
                                        if (!store[k]) v[k] = old[k];
                                }
                                __builtin_nontemporal_store(v, reinterpret_cast<v4h *>(o));
                            } else if (whole) {
                                __builtin_nontemporal_store(v, reinterpret_cast<v4h *>(o));
                            } else {
#pragma unroll
                                for (int k = 0; k < 4; ++k)
                                    if (store[k]) o[k] = v[k];
                            }
                        }
                        f += df; p += dp;
                        if (f >= DV) { f -= DV; ++p; }
                    }
                    return;
                }
                for (int q = tid; q < NQ; q += nthr) {
                    if constexpr (TO) {
                        if (prow != nullptr && p >= n_rows) {  // rows of absent observers: copied whole
                            const v4f v = *reinterpret_cast<const v4f *>(prow + 4 * (int64_t)q);
                            __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(orow + 4 * (int64_t)q));
                            f += df; p += dp;
                            if (f >= DV) { f -= DV; ++p; }
                            continue;
                        }
                    }
                    if (p >= n_rows) break;  // rows of absent observers keep their old contents
                    const int base = (obx[p] - obs_off + pad) * GW + (oby[p] - obs_off + pad);
                    float val[4];
                    bool keep[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t c = s_code[4 * f + k];
                        const uint32_t kind = c >> 24;
                        keep[k] = true;
                        val[k] = 0.0f;
                        if (kind == K_GRID) {
                            const uint32_t v = g_map[base + (int)(c & 0xFFFFFFu)];
                            keep[k] = v != PAD_CNT;
                            val[k] = s_vtab[v];
                        } else if (kind == K_ID) {
                            val[k] = (float)((double)p / (double)(LIVE ? np : d.P));  // :440-445
                        } else if (kind == K_FILL) {
                            val[k] = d.fill32;  // even obs_range: never-copied channel-0 cells
                        } else {
                            keep[k] = false;
                        }
                    }
                    float *o = orow + 4 * (int64_t)q;
                    if constexpr (TO) {
                        if (prow != nullptr) {  // one whole store; the kept elements from the previous buffer
                            v4f v = {val[0], val[1], val[2], val[3]};
                            if (!(keep[0] & keep[1] & keep[2] & keep[3])) {
                                const v4f old = *reinterpret_cast<const v4f *>(prow + 4 * (int64_t)q);
                                if (!keep[0]) v.x = old.x;
                                if (!keep[1]) v.y = old.y;
                                if (!keep[2]) v.z = old.z;
                                if (!keep[3]) v.w = old.w;
                            }
                            __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(o));
                            f += df; p += dp;
                            if (f >= DV) { f -= DV; ++p; }
                            continue;
                        }
                    }
                    if (keep[0] & keep[1] & keep[2] & keep[3]) {
                        const v4f v = {val[0], val[1], val[2], val[3]};
                        __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(o));
                    } else {
                        if (keep[0]) o[0] = val[0];
                        if (keep[1]) o[1] = val[1];
                        if (keep[2]) o[2] = val[2];
                        if (keep[3]) o[3] = val[3];
                    }
                    f += df; p += dp;
                    if (f >= DV) { f -= DV; ++p; }
                }
                return;
            }
            // dword path (rows that are not whole float4s: even obs_range with flatten)
            if constexpr (H16) {
                // binary16 buffers: 2-byte elements.  Two buffers: every element of all P rows, the step's value or the previous buffer's
                // 16 bits; in place: the elements the pass writes
                uint16_t *orow16 = reinterpret_cast<uint16_t *>(io.obs) + env * (int64_t)d.P * d.D;
                const uint16_t *prow16 = src ? reinterpret_cast<const uint16_t *>(src) + env * (int64_t)d.P * d.D : nullptr;
                for (int p = 0; p < (prow16 ? d.P : n_rows); ++p) {
                    const int base = p < n_rows ? (obx[p] - obs_off + pad) * GW + (oby[p] - obs_off + pad) : 0;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int r = tid + t * nthr;
                        if (r >= d.D) continue;
                        const uint32_t kind = code[t] >> 24;
                        bool store = false;
                        float val = 0.0f;
                        if (p < n_rows) {
                            if (kind == K_GRID) {
                                const uint32_t g = g_map[base + (int)(code[t] & 0xFFFFFFu)];
                                store = g != PAD_CNT;
                                val = s_vtab[g];
                            } else if (kind == K_ID) {
                                store = true;
                                val = (float)((double)p / (double)(LIVE ? np : d.P));
                            } else if (kind == K_FILL) {
                                store = true;
                                val = d.fill32;
                            }
                        }
                        if (store) orow16[p * d.D + r] = half_bits(val);
                        else if (prow16 != nullptr) orow16[p * d.D + r] = prow16[p * d.D + r];
                    }
                }
                return;
            }
            if constexpr (TO) {
                if (prow != nullptr) {  // every element of all P rows: the step's value, or the previous buffer's
                    for (int p = 0; p < d.P; ++p) {
                        const int base = p < n_rows ? (obx[p] - obs_off + pad) * GW + (oby[p] - obs_off + pad) : 0;
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            const int r = tid + t * nthr;
                            if (r >= d.D) continue;
                            const uint32_t kind = code[t] >> 24;
                            bool keep = false;
                            float val = 0.0f;
                            if (p < n_rows) {
                                if (kind == K_GRID) {
                                    const uint32_t v = g_map[base + (int)(code[t] & 0xFFFFFFu)];
                                    keep = v != PAD_CNT;
                                    val = s_vtab[v];
                                } else if (kind == K_ID) {
                                    keep = true;
                                    val = (float)((double)p / (double)(LIVE ? np : d.P));
                                } else if (kind == K_FILL) {
                                    keep = true;
                                    val = d.fill32;
                                }
                            }
                            orow[p * d.D + r] = keep ? val : prow[p * d.D + r];
                        }
                    }
                    return;
                }
            }
            for (int p = 0; p < n_rows; ++p) {
                const int base = (obx[p] - obs_off + pad) * GW + (oby[p] - obs_off + pad);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int r = tid + t * nthr;
                    const uint32_t kind = code[t] >> 24;
                    if (kind == K_GRID) {
                        const uint32_t v = g_map[base + (int)(code[t] & 0xFFFFFFu)];
                        if (v != PAD_CNT) orow[p * d.D + r] = s_vtab[v];
                    } else if (kind == K_ID) {
                        orow[p * d.D + r] = (float)((double)p / (double)(LIVE ? np : d.P));  // :440-445
                    } else if (kind == K_FILL) {
                        orow[p * d.D + r] = d.fill32;  // even obs_range: never-copied channel-0 cells
                    }
                }
            }
        };


        if (mode == 1) {
            // -------------------------------------------------------- grids for this env
            {
                const uint32_t *mt = reinterpret_cast<const uint32_t *>(d.maps + (int64_t)map_id * d.map_stride);
                const uint32_t *ct = reinterpret_cast<const uint32_t *>(d.cnt_tmpl);
                for (int k = tid; k < gsz_words; k += nthr) {
                    if (cached_map != map_id) reinterpret_cast<uint32_t *>(g_map)[k] = mt[k];
                    const uint32_t c = ct[k];
                    reinterpret_cast<uint32_t *>(g_pc)[k] = c;
                    reinterpret_cast<uint32_t *>(g_ec)[k] = c;
                    reinterpret_cast<uint32_t *>(g_cr)[k] = 0u;
                }
                cached_map = map_id;
            }
            __syncthreads();
            // -------------------------------------------------------- pre-move evader counts (:364-365)
            for (int i = tid; i < d.E; i += nthr) {
                if (!((s_gone[i >> 5] >> (i & 31)) & 1u))
                    lds_byte_add(g_ec, (s_ax[d.P + i] + pad) * GW + s_ay[d.P + i] + pad, &s_misc[3]);
            }
            __syncthreads();
            // proximity reward on the PRE-move state, np.clip keeps border pursuers on their
            // own cell (pursuit_evade.py:374-380)
            for (int p = tid; p < (LIVE ? np : d.P); p += nthr) {
                const int x = s_ax[p], y = s_ay[p];
                const int xm = max(x - 1, 0), xp = min(x + 1, d.xs - 1);
                const int ym = max(y - 1, 0), yp = min(y + 1, d.ys - 1);
                s_kpre[p] = (int)g_ec[(xm + pad) * GW + y + pad] + (int)g_ec[(xp + pad) * GW + y + pad] +
                            (int)g_ec[(x + pad) * GW + yp + pad] + (int)g_ec[(x + pad) * GW + ym + pad];
            }
            __syncthreads();
            // -------------------------------------------------------- moves (:229-241)
            for (int a = tid; a < d.A; a += nthr) {
                const bool is_p = a < d.P;
                const int i = a - d.P;
                if (!is_p && ((s_gone[i >> 5] >> (i & 31)) & 1u)) continue;
                if (LIVE && is_p && a >= np) continue;  // a pursuer slot this episode does not have
                int x = s_ax[a], y = s_ay[a];
                int act;
                int k = 0;  // evaders: index in the evader LAYER = alive evaders in slots below i
                if (!is_p) {
                    lds_byte_sub(g_ec, (x + pad) * GW + y + pad);  // undo the pre-move count
                    for (int w = 0; w < (i >> 5); ++w) k += 32 - __popc(s_gone[w]);
                    k += (i & 31) - __popc(s_gone[i >> 5] & ((1u << (i & 31)) - 1u));
                }
                if (d.train_pursuit) {
                    if (is_p) {
                        act = io.actions[env * d.P + a];
                    } else if (io.inj_eact != nullptr) {
                        act = io.inj_eact[env * d.E + k];
                    } else act = pr::evader_action(gid, tick, (uint32_t)k, d.k0, d.k1);
                } else {
                    // evader control (:215-224): action k moves the k-th agent of the evader layer (`for i, a in enumerate(actions):
                    // agent_layer.move_agent(i, a)`, :229-230; the caller passes one action per env.agents entry = n_pursuers of
                    // them, so evaders past the first n_pursuers of the layer never move); every pursuer moves by one
                    // pursuer_controller.act() draw (:238-241), injected as entry a of inj_eact [n_envs][P]
                    if (!is_p) {
                        act = k < d.P ? io.actions[env * d.P + k] : 4;
                    } else if (io.inj_eact != nullptr) {
                        act = io.inj_eact[env * d.P + a];
                    } else act = pr::pursuer_action(gid, tick, (uint32_t)a, d.k0, d.k1);
                }
                // DiscreteAgent.step, DiscreteAgent.py:69-97
                const bool term = (s_term[a >> 5] >> (a & 31)) & 1u;
                if (!term) {
                    if (g_map[(x + pad) * GW + y + pad] == 1) {
                        atomicOr(&s_term[a >> 5], 1u << (a & 31));  // standing in a building
                    } else {
                        int nx = x, ny = y;
                        if (act == 0) nx = x - 1;
                        else if (act == 1) nx = x + 1;
                        else if (act == 2) ny = y + 1;
                        else if (act == 3) ny = y - 1;
                        // padded map layer: 0 = free, 1 = building, 0xFE = outside the map
                        if (g_map[(nx + pad) * GW + ny + pad] == 0) {
                            x = nx;
                            y = ny;
                        }
                    }
                }
                s_ax[a] = (uint8_t)x;
                s_ay[a] = (uint8_t)y;
                lds_byte_add(is_p ? g_pc : g_ec, (x + pad) * GW + y + pad, &s_misc[3]);  // :244-246
            }
            __syncthreads();
            // -------------------------------------------------------- catch resolution (:463-521)
            const uint8_t *need_tab = d.maps + (int64_t)map_id * d.map_stride + GSZ;
            for (int i = tid; i < d.E; i += nthr) {
                if ((s_gone[i >> 5] >> (i & 31)) & 1u) continue;
                const int x = s_ax[d.P + i], y = s_ay[d.P + i];
                const int c0 = (x + pad) * GW + y + pad;
                bool caught;
                if (d.surround) {
                    // neighbour order of surround_mask (:150); pad cells hold 0xFF => never a hit
                    const bool h0 = (uint8_t)(g_pc[c0 - GW] - 1) < 0xFEu;
                    const bool h1 = (uint8_t)(g_pc[c0 + GW] - 1) < 0xFEu;
                    const bool h2 = (uint8_t)(g_pc[c0 + 1] - 1) < 0xFEu;
                    const bool h3 = (uint8_t)(g_pc[c0 - 1] - 1) < 0xFEu;
                    const int cnt = (int)h0 + (int)h1 + (int)h2 + (int)h3;
                    caught = (cnt == (int)need_tab[x * d.ys + y]);  // need_to_surround :523-540
                    if (caught) {  // pursuers standing on a matched neighbour get credit (:489-495)
                        if (h0) g_cr[c0 - GW] = 1;
                        if (h1) g_cr[c0 + GW] = 1;
                        if (h2) g_cr[c0 + 1] = 1;
                        if (h3) g_cr[c0 - 1] = 1;
                    }
                } else {
                    caught = (int)g_pc[c0] >= d.n_catch;  // :498
                    if (caught) g_cr[c0] = 1;             // :503-506
                }
                if (caught) {
                    atomicOr(&s_gone[i >> 5], 1u << (i & 31));
                    atomicAdd(&s_misc[4], 1u);
                }
            }
            __syncthreads();
            // -------------------------------------------------------- rewards (:254-262)
            int n_alive = d.E;
            for (int w = 0; w < d.ngw; ++w) n_alive -= __popc(s_gone[w]);
            for (int p = tid; p < d.P; p += nthr) {
                if (LIVE && p >= np) {  // no such pursuer: reward 0
                    io.rew[env * d.P + p] = 0.0f;
                    continue;
                }
                const int sur = g_cr[(s_ax[p] + pad) * GW + s_ay[p] + pad];
                const double catchr = d.catchr_env ? d.catchr_env[env] : d.catchr;
                const double r = pr::pursuer_reward(catchr, s_kpre[p], d.term_pursuit, sur, d.urgency);
                if (d.reward_global) s_rew[p] = r;
                else io.rew[env * d.P + p] = (float)r;
            }
            if (d.reward_global) {
                __syncthreads();
                if (tid < (LIVE ? np : d.P)) {
                    const double m = np_pairwise_sum(s_rew, LIVE ? np : d.P) / (double)(LIVE ? np : d.P);
                    for (int p = tid; p < (LIVE ? np : d.P); p += nthr) io.rew[env * d.P + p] = (float)m;
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

        if (mode == 1 && do_reset) {
            // auto-reset: the reference sequence is step() then reset(); both write the persistent
            // observation buffer, and cells the second write skips keep the first one's values
            write_obs(obs_prev);
            __syncthreads();
        }
        if (do_reset) {
            // ---------------------------------------------------------- reset (:173-207)
            __syncthreads();
            if (tid == 0) s_misc[3] = 0u;                            // a new episode: the overflow mark goes
            for (int w = tid; w < d.ngw; w += nthr) s_gone[w] = 0u;  // :175-176
            for (int w = tid; w < d.ntw; w += nthr) s_term[w] = 0u;  // fresh agents
            if (io.inj_map != nullptr && mode == 0) map_id = io.inj_map[env];
            else if (d.sample_maps) map_id = pr::reset_map_id(gid, tick, d.k0, d.k1, d.n_maps);
            {
                const uint32_t *mt = reinterpret_cast<const uint32_t *>(d.maps + (int64_t)map_id * d.map_stride);
                const uint32_t *ct = reinterpret_cast<const uint32_t *>(d.cnt_tmpl);
                for (int k = tid; k < gsz_words; k += nthr) {
                    if (cached_map != map_id) reinterpret_cast<uint32_t *>(g_map)[k] = mt[k];
                    const uint32_t c = ct[k];
                    reinterpret_cast<uint32_t *>(g_pc)[k] = c;
                    reinterpret_cast<uint32_t *>(g_ec)[k] = c;
                }
                cached_map = map_id;
            }
            const pr::Window win = pr::reset_window(gid, tick, d.k0, d.k1, d.cw_env ? d.cw_env[env] : d.cw, d.xs, d.ys);
            const bool inj = io.inj_pos != nullptr && mode == 0;   // (an injected position with x < 0 marks an evader slot that is not created)
            int n_create = d.E;
            if constexpr (LIVE) {  // the pending counts take effect
                const pr::Counts live = pr::clamp_pending(pending[2 * env], pending[2 * env + 1], d.P, d.E);
                np = live.np, ne = n_create = live.ne;
            }
            if (d.max_opponents > 0 && !inj) n_create = pr::reset_n_create(gid, tick, d.k0, d.k1, d.max_opponents, LIVE ? ne : d.E);
            __syncthreads();
            for (int a = tid; a < d.A; a += nthr) {  // create_agents, agent_utils.py:12-28
                int x = 0, y = 0;
                if (LIVE && ((a < d.P && a >= np) || a - d.P >= ne)) {  // a slot this episode does not have
                    if (a >= d.P) atomicOr(&s_gone[(a - d.P) >> 5], 1u << ((a - d.P) & 31));
                    s_ax[a] = NOT_HERE;
                    s_ay[a] = NOT_HERE;
                    continue;
                }
                if (a >= d.P && (a - d.P >= n_create || (inj && io.inj_pos[(env * d.A + a) * 2] < 0))) {
                    atomicOr(&s_gone[(a - d.P) >> 5], 1u << ((a - d.P) & 31));
                    s_ax[a] = 0;
                    s_ay[a] = 0;
                    continue;
                }
                if (io.inj_pos != nullptr && mode == 0) {
                    x = io.inj_pos[(env * d.A + a) * 2];
                    y = io.inj_pos[(env * d.A + a) * 2 + 1];
                } else {
                    for (uint32_t att = 0; att < 1024u; ++att) {   // bounded, like the oracle's
                        const uint32_t aidx = LIVE ? pr::live_agent_index(a, d.P, np) : (uint32_t)a;
                        const pr::Cell c = pr::reset_cell(gid, tick, aidx, att, d.k0, d.k1, win);
                        x = c.x, y = c.y;
                        if (g_map[(x + pad) * GW + y + pad] != 1) break;
                    }
                }
                s_ax[a] = (uint8_t)x;
                s_ay[a] = (uint8_t)y;
                lds_byte_add(a < d.P ? g_pc : g_ec, (x + pad) * GW + y + pad, &s_misc[3]);  // :201-203
            }
            tick += 1;
            tstep = 0;
            __syncthreads();
        }

        write_obs(mode == 1 && do_reset ? nullptr : obs_prev);  // (after a fused reset: in place, over the step pass's rows)
        // -------------------------------------------------------------- store state record
        for (int a = tid; a < d.A; a += nthr)
            reinterpret_cast<uint16_t *>(rec + HDR_BYTES)[a] = (uint16_t)(s_ax[a] | (s_ay[a] << 8));
        for (int w = tid; w < d.ngw; w += nthr) reinterpret_cast<uint32_t *>(rec + d.off_gone)[w] = s_gone[w];
        for (int w = tid; w < d.ntw; w += nthr) reinterpret_cast<uint32_t *>(rec + d.off_term)[w] = s_term[w];
        if (tid == 0) {
            uint32_t *h = reinterpret_cast<uint32_t *>(rec);
            h[0] = tick;
            h[1] = (uint32_t)tstep;
            h[2] = (uint32_t)map_id;
            h[3] = s_misc[3];   // sticky count-overflow mark of the episode (0 in every run that stays inside the byte grids)
        }
    }
