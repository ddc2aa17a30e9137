"""The structure / input fuzzers of tests/dev (seeded, deterministic) as gates of the -m gpu suite: a short seed range of each, every case
against the oracle.  The long ranges and what they found are in profiles/r05_fuzz_*.txt; a seed range here is one that is clean there
(fuzz_solve seed 9 -- 290 ragged landmarks, final inverse depths 1.6e-6 apart after eight iterations -- and the exactly-collinear detections
of fuzz_lines scenes 0, 1, 6 are outside them; DESIGN.md 2 says why those are not defects)."""
import importlib
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

DEV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev")


def run(module, *argv):
    sys.path.insert(0, DEV)
    try:
        m = importlib.import_module(module)
        old = sys.argv
        sys.argv = [module + ".py"] + [str(a) for a in argv]
        try:
            return m.main()
        finally:
            sys.argv = old
    finally:
        sys.path.remove(DEV)


def test_window_structures_solved_four_ways_and_in_mixed_batches(gpu):
    assert run("fuzz_solve", 120, 10) == 0


def test_window_structures_solved_to_convergence(gpu):
    """the same structures with the convergence tests on, (50, to convergence) on the device and in the oracle: the function and parameter
    tolerances and the iteration limit decide where a solve ends (the oracle alone over seeds 10 .. 129: 90 / 1 / 29).  In both modes a
    `trace` verdict counts as a mismatch unless the oracle's own trace moves under 1e-13 noise, and at most 5 % of a setting's cases may
    be `trace` (tests/dev/fuzz_solve.py)."""
    assert run("fuzz_solve", 24, 10, "convergence") == 0


def test_marginalisation_of_the_fuzz_structures(gpu):
    assert run("fuzz_marg", 150, 0) == 0


def test_time_offset_windows_on_the_fuzz_structures(gpu):
    assert run("fuzz_td", 8, 0) == 0


def test_line_association_on_random_scenes(gpu):
    assert run("fuzz_lines", 20, 7) == 0


def test_preintegration_on_random_streams(gpu):
    assert run("fuzz_preint", 15, 0) == 0


def test_gauge_fix_on_random_windows(gpu):
    assert run("fuzz_gauge", 600, 0) == 0


def test_factor_evaluators_on_random_inputs(gpu):
    assert run("fuzz_factors", 500, 0) == 0


def test_pose_graphs_on_random_structures(gpu):
    """200 seeded graphs, each alone and sixteen at a time in ragged batches (tests/test_pose_graph_cpu.py holds the same seed range to
    decisions 1 % clear of their thresholds on the oracle alone)"""
    assert run("fuzz_pose_graph", 200, 0) == 0


def test_visual_inertial_alignment_on_random_sequences(gpu):
    """60 seeded sequences, each alone and sixteen at a time in ragged batches, against the restatement on the device's own pre-integrations
    (tests/test_vi_alignment_cpu.py holds the same seed range decided by the restatement alone)"""
    assert run("fuzz_vi_alignment", 60, 0) == 0


def test_native_estimator_on_stress_streams(gpu):
    assert run("fuzz_estimator", 6, 0, 40) == 0
