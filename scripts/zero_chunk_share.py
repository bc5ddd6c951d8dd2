"""CPU only (the C oracle and numpy): which share of the headline step's observation chunks the "zeros over known zeros" rule of the
one-wavefront Pursuit kernel (madrl_amd/csrc/pursuit_wave.hpp, Shape::ZSKIP) can leave unstored.

The kernel's own eligibility is replayed, not the oracle's knowledge: a cell is "known zero" only through the stale-zero mask bit the
kernel keeps for it (a stored cell: value != 0; a cell outside the map: its old bit), the bit position a lane's 16 bits leave out
(pursuit_zm16.hpp, drop_slot) always reads "unknown", and a 64-byte chunk -- four float4 slots, one per lane of an aligned quad -- is
skipped iff the parent rule would have stored it (a clean slot with a cell inside the map) and no slot of it has an old bit set or a
non-zero new value.  Both passes of a fused auto-reset count.  For comparison the script also counts the chunks that hold only zeros
before and after a pass whatever the masks say (what an all-knowing rule could skip).

Actions as bench.py draws them: 16 random action tensors used in turn, so every pursuer repeats a 16-step walk and drifts (until a wall
stops it) -- the windows of a long run lie against the walls more often than under fresh random actions, and bench.py times steps
2 000 and later.  `iid` as the fourth argument draws fresh actions at every step instead.

  python scripts/zero_chunk_share.py [n_envs=256] [first_step=2000] [last_step=2100] [cycle16|iid]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XS = YS = 16
P, E, R, H = 8, 30, 7, 500          # bench.py's headline: episodes of 500 steps, ages uniform at the start
D = 3 * R * R + 1
DV = D // 4
NQ = P * DV
NS = (NQ + 63) // 64
OFF = (R - 1) // 2


def useful(q):   # pursuit_zm16.hpp: float4 slot q holds a cell of channel 1 or 2
    m = q % DV
    return q < NQ and 4 * m + 3 >= R * R and 4 * m < 3 * R * R


def drop_slot(lane):
    d = -1
    for s in range(NS if NS == 5 else 0):
        if not useful(lane + 64 * s):
            d = s
    return d


def main():
    from madrl_amd.maps import rectangle_map
    from oracle import pursuit as po
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    t0 = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    t1 = int(sys.argv[3]) if len(sys.argv) > 3 else 2100
    iid = len(sys.argv) > 4 and sys.argv[4] == "iid"
    orc = po.PursuitOracle([rectangle_map(XS, YS)], n_envs=N, seed=0, n_pursuers=P, n_evaders=E, obs_range=R, n_catch=2, surround=True,
                           flatten=True, reward_mech="local")
    dropped = np.zeros(NQ, bool)   # slots whose mask bits are not kept
    for q in range(NQ):
        dropped[q] = drop_slot(q % 64) == q // 64
    dropped_cell = np.repeat(dropped, 4)[None, :]
    ii, jj = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")

    def stored_cells():
        """[N, P * D] the cells the current pass stores: channel 0 and the id always, channels 1 and 2 where the window cell is inside the map"""
        pos = orc.get_state()["pos_p"]
        gx, gy = pos[:, :, 0, None, None] - OFF + ii, pos[:, :, 1, None, None] - OFF + jj
        inside = ((gx >= 0) & (gx < XS) & (gy >= 0) & (gy < YS)).reshape(N, P, R * R)
        st = np.ones((N, P, D), bool)
        st[:, :, R * R:2 * R * R] = inside
        st[:, :, 2 * R * R:3 * R * R] = inside
        return st.reshape(N, P * D)

    bits = np.zeros((N, P * D), bool)        # the library declares its freshly allocated buffer all-zero
    tot = dict(passes=0, chunks=0, parent_nt_bytes=0, parent_chunks=0, skipped=0, skipped_clean_bytes=0, all_zero=0, all_zero_with_dropped=0)

    def one_pass(before, count, sel):
        """one observation pass of the envs `sel`: count what the rules do with its chunks, then update the mask bits"""
        n = int(sel.sum())
        after, was = orc.obs.reshape(N, P * D)[sel], before.reshape(N, P * D)[sel]
        st, b = stored_cells()[sel], bits[sel]
        nz = after != 0
        if count:
            slot = lambda c: c.reshape(n, NQ, 4).any(-1)
            chunk = lambda c: c.reshape(n, NQ // 4, 4)
            dirty = slot(~st & b)                                   # a cell outside the map that may hold a value: dword stores
            a = chunk(slot(st) & ~dirty).any(-1)                    # the parent rule: the chunk's clean slots are stored
            x = slot(b | dropped_cell | (st & nz))                  # an old bit (a dropped position: always), or a non-zero value stored now
            skip = a & ~chunk(x).any(-1)
            # the kernel's form of the rule asks the CLEAN slots only (a dirty slot stores its inside cells one by one whatever the others
            # do): the clean slots of a chunk are not stored iff none of them has an x -- a chunk with a dirty slot included
            skip_clean = a & ~chunk(x & ~dirty).any(-1)
            tot["skipped_clean_bytes"] += 16 * int((chunk(~dirty).sum(-1) * skip_clean).sum())
            assert not bool((skip & ~skip_clean).any())
            zz = ~chunk(slot(was != 0) | slot(nz)).any(-1)
            assert not bool((skip & ~zz).any()), "the rule skipped a chunk that does not hold zeros before and after"
            tot["passes"] += n
            tot["chunks"] += a.size
            tot["parent_chunks"] += int(a.sum())
            tot["parent_nt_bytes"] += 16 * int((chunk(~dirty).sum(-1) * a).sum())
            tot["skipped"] += int(skip.sum())
            tot["all_zero"] += int(zz.sum())
            tot["all_zero_with_dropped"] += int((zz & chunk(np.broadcast_to(dropped[None, :], (n, NQ))).any(-1)).sum())
        bits[sel] = np.where(st, nz, b)

    rng = np.random.RandomState(0)
    everyone = np.ones(N, bool)
    orc.reset()
    one_pass(np.zeros_like(orc.obs), False, everyone)
    age = rng.randint(H, size=N)
    env_steps = 0
    cycle = [rng.randint(5, size=(N, P)) for _ in range(16)]
    for t in range(t1):
        count = t >= t0
        before = orc.obs.copy()
        _, _, done, _ = orc.step(rng.randint(5, size=(N, P)) if iid else cycle[t % 16])
        one_pass(before, count, everyone)
        age += 1
        sel = (done != 0) | (age >= H)
        if sel.any():   # the second pass of a fused auto-reset, in the envs that run it
            before = orc.obs.copy()
            orc.reset(mask=sel.astype(np.uint8))
            one_pass(before, count, sel)
            age[sel] = 0
        env_steps += N if count else 0
    row = 4 * P * D
    print("PursuitEvade %dx%d, %d v %d, obs_range %d, flatten: %d envs, steps %d..%d, %s actions, %d env-steps, %d passes"
          % (XS, YS, P, E, R, N, t0, t1, "fresh random" if iid else "16 random action tensors in turn (bench.py)", env_steps, tot["passes"]))
    print("chunks per env and pass: %d (row bytes %d)" % (NQ // 4, row))
    print("chunks the parent stores (a clean slot with a cell inside the map): %.2f %% of all" % (100.0 * tot["parent_chunks"] / tot["chunks"]))
    print("chunks all-zero before and after a pass (an all-knowing rule):       %.2f %% of all, %.2f %% of them hold a dropped mask position"
          % (100.0 * tot["all_zero"] / tot["chunks"], 100.0 * tot["all_zero_with_dropped"] / max(tot["all_zero"], 1)))
    print("chunks no slot of which has an x:                                     %.2f %% of all" % (100.0 * tot["skipped"] / tot["chunks"]))
    quad = 64.0 * tot["skipped"] / env_steps
    print("whole chunks only (no slot of the chunk, dirty ones included, has an x): %.1f of %d row bytes per env-step = %.2f %%; at 65 536 envs: %.2f MB per step"
          % (quad, row, 100.0 * quad / row, quad * 65536 / 1e6))
    saved = float(tot["skipped_clean_bytes"]) / env_steps
    print("the kernel's rule (no CLEAN slot of the chunk has an x):                  %.1f of %d row bytes per env-step = %.2f %%; at 65 536 envs: %.2f MB per step"
          % (saved, row, 100.0 * saved / row, saved * 65536 / 1e6))
    print("predicted_share %.4f predicted_MB_per_step_65536 %.2f" % (saved / row, saved * 65536 / 1e6))


if __name__ == "__main__":
    main()
