"""bench.py's option handling (no GPU): a plain run switches off every leg beyond the headline figure, --full keeps
them as the options say."""
import importlib.util
import os

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_skips_every_extra_leg(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--latency-iters", "50", "--dump-outputs", "d"])
    assert not a.full and a.no_cpu and a.no_verify
    for k in bench.EXTRA_LEGS:
        assert getattr(a, k) == 0, k
    # what the timed steps and the dump depend on is untouched
    assert (a.gpus, a.steps, a.warmup, a.batch, a.rounds, a.unique, a.streams, a.mode, a.dump_outputs) == (1, 7, 2, 256, 8, 16, 0, "batch", "d")


def test_full_run_keeps_the_legs_as_given(bench):
    plain = bench.parse_args(["--steps", "7"])
    full = bench.parse_args(["--steps", "7", "--full", "--latency-iters", "50", "--no-cpu"])
    assert full.full and full.no_cpu and not full.no_verify
    assert full.latency_iters == 50
    defaults = bench.parse_args(["--full"])
    for k in bench.EXTRA_LEGS:
        if k != "latency_iters":
            assert getattr(full, k) == getattr(defaults, k) > 0, k
    # the legs' options are the only difference between a plain and a full parse
    diff = {k for k in vars(full) if vars(full)[k] != vars(plain)[k]}
    assert diff <= set(bench.EXTRA_LEGS) | {"full", "no_cpu", "no_verify"}, diff
