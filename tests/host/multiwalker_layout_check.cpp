// multiwalker_layout_check.cpp -- the state-buffer layout of a MultiWalker handle (madrl_amd/csrc/multiwalker_layout.hpp) on a CPU.
// tests/test_multiwalker_layout_cpu.py compiles this once per capacity class (-DMW_CAPW=4 / 8 / 10 with -DMW_NLANES=4 / 8 / 16) with
// -fsanitize=address,undefined and runs it.  For every n_walkers the class holds, one_hot 0 and 1 and a few batch sizes it checks that
// the regions lie in order without overlap, start aligned and end exactly at `total`, and prints one line
// "n_walkers one_hot n_envs total world_dw" for the test to compare with the sizes recorded from the library before the layout had a
// function of its own.
#include <stdio.h>

#include "../../madrl_amd/csrc/multiwalker_layout.hpp"

namespace {

int failures = 0;

#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ++failures;                                                                  \
            fprintf(stderr, "W=%d one_hot=%d n_envs=%lld: ", W, one_hot, (long long)n); \
            fprintf(stderr, __VA_ARGS__);                                                \
            fprintf(stderr, "\n");                                                       \
        }                                                                                \
    } while (0)

void check(int W, int one_hot, int64_t n) {
    mw::Model M;
    mw::host_model(M, W);
    const mw::MwLayout L = mw::mw_layout(M, one_hot, n);
    const uint64_t N = (uint64_t)n, rec = (uint64_t)L.world_dw * 4;
    // every region with the bytes the kernels use of it, in the order of the buffer
    const struct { const char *name; uint64_t at, bytes, align; } r[] = {
        {"records", L.records, rec * N, 16},
        {"pending", L.pending, N, 1},
        {"spare_state", L.spare_state, rec * N, 16},
        {"spare_obs", L.spare_obs, (uint64_t)W * (uint64_t)mw::host_obs_dim(one_hot) * 4 * N, 16},
        {"ready_step", L.ready_step, 4 * N, 4},
        {"dirty_list", L.dirty_list, 2 * 4 * N, 4},
        {"n_dirty", L.n_dirty, 2 * 4, 4},
        {"step_count", L.step_count, 4, 4},
    };
    const int R = (int)(sizeof(r) / sizeof(r[0]));
    CHECK(L.records == 0, "the records start the buffer, not at %llu", (unsigned long long)L.records);
    for (int k = 0; k < R; ++k) {
        CHECK(r[k].at % r[k].align == 0, "%s at %llu is not %llu-byte aligned", r[k].name, (unsigned long long)r[k].at, (unsigned long long)r[k].align);
        if (k + 1 < R) CHECK(r[k].at + r[k].bytes <= r[k + 1].at, "%s [%llu, +%llu) runs into %s at %llu", r[k].name, (unsigned long long)r[k].at,
                             (unsigned long long)r[k].bytes, r[k + 1].name, (unsigned long long)r[k + 1].at);
    }
    // the four trailing dwords: n_dirty[2], step_count, one unused -- and nothing behind them
    CHECK(L.n_dirty == L.dirty_list + 8 * N, "the four dwords follow the lists");
    CHECK(L.step_count == L.total - 8 && L.n_dirty == L.total - 16, "step_count is the third of the four trailing dwords, which end at total");
    // one record: mw::World, the schedule and the manifold pool, whole 16-byte words
    CHECK(L.scratch_off_dw * 4 >= (int)sizeof(mw::World) && L.scratch_off_dw % 4 == 0, "the scratch starts behind the world at a 16-byte boundary");
    CHECK(L.world_dw == L.scratch_off_dw + L.scratch_bytes / 4 && L.scratch_bytes % 16 == 0, "a record is the world and its scratch");
    CHECK(L.scratch_bytes >= mw::SOLVE_HDR_BYTES + M.max_manifolds * (int)sizeof(mw::Manifold), "the pool holds max_manifolds manifolds");
    CHECK((size_t)L.cold_q * 16 <= sizeof(mw::Cold) + 15 && (size_t)L.cold_q * 16 >= offsetof(mw::Cold, slot) + (size_t)M.n_slots * sizeof(mw::Slot),
          "cold_q covers the contact slots in use and stays inside mw::Cold");
    printf("%d %d %lld %llu %d\n", W, one_hot, (long long)n, (unsigned long long)L.total, L.world_dw);
}

}  // namespace

int main() {
    const int64_t batches[] = {1, 15, 16, 17, 16384};
    for (int W = 1; W <= mw::MAX_WALKERS; ++W)
        for (int one_hot = 0; one_hot < 2; ++one_hot)
            for (int64_t n : batches) check(W, one_hot, n);
    if (failures) fprintf(stderr, "%d layout checks failed\n", failures);
    return failures ? 1 : 0;
}
