"""CPU side of tests/test_gpu_entry_paths.py: the inputs of those tests must DISCRIMINATE -- a GPU test that cannot tell a present second attempt
from a missing one is worthless -- and the lane emulators of the kernel text (one wave, pairs, teams) must follow the oracle on them, so that the
CPU suite sees what the batch kernels call.  The sets: tests/entry_path_sets.py."""
import numpy as np
import pytest

from tests import entry_path_sets as eps
from tests.emu import emu

ROWS = sorted(eps.ORACLE_COUNTS)


@pytest.mark.parametrize("name,mode", ROWS)
def test_the_oracle_still_gives_the_pinned_verdicts_on_the_sets(name, mode):
    """Status counts of the oracle with and without the second attempt, as recorded when the sets were chosen: if the generator, a fixture or a
    default moves, this fails before a GPU test silently stops testing anything."""
    off, on = eps.ORACLE_COUNTS[(name, mode)]
    assert eps.counts(eps.oracle(name, mode, 0)["status"]) == off
    assert eps.counts(eps.oracle(name, mode, 100)["status"]) == on


def test_the_recorded_iteration_counts_of_the_oracle():
    a0, a1, d0, d1 = eps.oracle("A", 0, 100)["iters"], eps.oracle("A", 1, 100)["iters"], eps.oracle("D", 1, 0)["iters"], eps.oracle("D", 1, 100)["iters"]
    assert abs(a0.mean() - 68.9) < 0.05 and a0.max() == 112 and abs(a1.mean() - 41.0) < 0.05 and a1.max() == 69
    assert d0.sum() == 2052 and d1.sum() == 3269


@pytest.mark.parametrize("name,mode", ROWS)
def test_the_second_attempt_changes_the_oracles_answer_on_every_discriminating_row(name, mode):
    """Status or iterations differ between cap 0 and cap 100 -- except on the rows listed in CAP_CHANGES_NOTHING (all converge in the first attempt with
    the full restoration phase), where both must be identical: those rows check that a cap does no harm."""
    r0, r1 = eps.oracle(name, mode, 0), eps.oracle(name, mode, 100)
    same = np.array_equal(r0["status"], r1["status"]) and np.array_equal(r0["iters"], r1["iters"])
    assert same == ((name, mode) in eps.CAP_CHANGES_NOTHING)
    if name == "D":      # statuses stay, the status-2 rows report the sum of both attempts
        s2 = r0["status"] == 2
        assert np.array_equal(r0["status"], r1["status"]) and (r1["iters"][s2] > r0["iters"][s2]).all() and np.array_equal(r1["iters"][~s2], r0["iters"][~s2])


@pytest.mark.parametrize("cap", [0, 100])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["B", "C", "C'"])
def test_one_wave_emulator_against_the_oracle(name, mode, cap):
    """The kernel text as the one-wave batch kernels call it (wave_solve_retry, status-4 hand-over to the restoration kernel's call) on a jam (C)
    and a numerical breakdown (C') in the S > 4 instantiation and on B: the oracle's statuses, iterations within 2 (the project's margin for the G12
    starts, test_far_off_cold_starts_of_other_sizes).  Measured gap: 0 on every row of B and C, 1 on one row of C' (modes 0 and 2, both caps) --
    tests/test_gpu_entry_paths.py sets its margin for C / C' from that (1 + 2)."""
    P, X, N, S, dt = eps.problem_set(name)
    ref = eps.oracle(name, mode, cap)
    e = emu.solve(P, X, N, S, dt, opts=emu.default_opts(restoration=mode, start_rollout=0, retry_cap=cap))
    gap = np.abs(e["iters"] - ref["iters"])
    print(f"\n{name} mode {mode} cap {cap}: emulator vs oracle iteration gap max {gap.max()} {gap.tolist()}")
    assert np.array_equal(e["status"], ref["status"]) and gap.max() <= 2
    ok = ref["status"] == 0
    if ok.any():
        assert eps.rms_q(e["x"][ok], ref["x"][ok], N).max() < 1e-5


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("nw", [4, "pair"])
def test_team_and_pair_emulators_make_the_second_attempt(nw, mode):
    """Set B through the multi-wave text with retry_cap = 100: the team build of tests/emu/bmpc_emu.cpp calls wave_solve_retry like the pair / team batch kernel
    (bmpc_multi_batch.inl).  Without the second attempt 11 of the 12 rows end as status 2; with it the oracle's statuses and iterations (within 2)."""
    P, X, N, S, dt = eps.problem_set("B")
    ref, ref0 = eps.oracle("B", mode, 100), eps.oracle("B", mode, 0)
    e = emu.solve_team(P, X, N, S, dt, nw=nw, opts=emu.default_opts(restoration=mode, start_rollout=0, retry_cap=100))
    e0 = emu.solve_team(P, X, N, S, dt, nw=nw, opts=emu.default_opts(restoration=mode, start_rollout=0, retry_cap=0))
    assert np.array_equal(e["status"], ref["status"]) and np.abs(e["iters"] - ref["iters"]).max() <= 2, (e["status"], e["iters"], ref["iters"])
    assert np.array_equal(e0["status"], ref0["status"]) and (e0["status"] == 2).sum() == 11 and np.abs(e0["iters"] - ref0["iters"]).max() <= 2
    ok = ref["status"] == 0
    assert eps.rms_q(e["x"][ok], ref["x"][ok], N).max() < 1e-5


# what the library's option record (csrc/bmpc_wave.inl Opts, read through the emulator) and the oracle's (oracle/bmpc_oracle.c) both have
SHARED_OPTION_FIELDS = ("tol", "max_iter", "mu_init", "mu_min_fac", "slack_push", "exact_hessian", "mu_warm", "stall_window", "restoration", "resto_short",
                        "resto_cap", "start_rollout", "hold_mu", "retry_cap", "bound_margin")


@pytest.mark.parametrize("N", [1, 11, 12, 40])
def test_the_library_and_the_oracle_state_the_same_horizon_rule(N):
    """The defaults of a handle of horizon N exist once per implementation -- bmpc_opts_for (csrc/bmpc_args.h; what bmpc_create, bmpc_default_options_for
    and the emulators run) and c_oracle.opts_for, an independent restatement -- and nothing else holds them together: on both sides of the cliff at
    N = 11 / 12 and at the ends of the range they agree on every field both records have.  Literals on both sides: equality, no tolerance."""
    from oracle import c_oracle
    lib, ora = emu.opts_for(N), c_oracle.opts_for(N)
    assert {f for f, _ in ora._fields_} - {"verbose"} == set(SHARED_OPTION_FIELDS) <= {f for f, _ in lib._fields_}
    for f in SHARED_OPTION_FIELDS:
        assert getattr(lib, f) == getattr(ora, f), (N, f, getattr(lib, f), getattr(ora, f))
    if N == 11:
        d = emu.default_opts()
        for f, _ in emu.Opts._fields_:
            assert getattr(d, f) == getattr(lib, f), f
