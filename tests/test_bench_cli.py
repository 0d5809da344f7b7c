"""bench.py's plain run does only what its headline figure needs; the roofline pass, the table materialisation timing, the
parity relay and the CPU baseline run only under --full, which is off by default."""
import sys

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_opt_in(monkeypatch):
    plain = _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert plain.full is False
    assert (plain.steps, plain.warmup) == (5, 2)
    full = _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2", "--full")
    assert full.full is True
    # the switches that trim the --full extras keep their defaults
    assert (full.no_cpu_baseline, full.profile_steps) == (False, 2)
