"""GPU tests (-m gpu): a Pursuit handle walked through every ordered pair of API calls (tests/pursuit_walk.py), each op replayed on the
CPU model and on the device, and after every op every observation slot, the guard bands, the launch outputs and the kernel entry compared
with the model bit for bit.  tests/test_pursuit_walk_cpu.py holds the conditions that keep these walks from being empty."""
import pytest

import pursuit_walk as pw

pytestmark = pytest.mark.gpu

CASES = [(name, seed) for name in pw.HANDLES for seed in pw.HANDLES[name]["seeds"]]


@pytest.mark.parametrize("name,seed", CASES)
def test_walk_through_the_c_abi_equals_the_model(name, seed):
    model = pw.model_for(name, seed)
    pw.replay(pw.make_env(name, seed), model, pw.walk(pw.kinds_of(name), seed, name))


@pytest.mark.parametrize("seed", pw.PY_SEEDS)
@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_walk_through_batched_pursuit_evade_equals_the_model(half, seed):
    model = pw.model_for("XF_c1", seed, half)
    pw.replay(pw.make_env("XF_c1", seed, half), model, pw.walk(pw.PY_KINDS, seed, "XF_c1", half), python=True)
