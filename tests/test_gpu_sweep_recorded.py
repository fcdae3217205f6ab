"""Recorded behaviour of the sorted sweep: the batches of tests/sweep_recorded.py replayed and compared, field for field, with what the
commit named in tests/golden/sweep_recorded.json computed (tools/sweep_record.py wrote it): every field of the result summary, a
digest of fetch(), and launches and algorithmic bytes of the locate, partition, resolve, expand and sort kernel classes.  The counters
pin what positions alone would not: the sequence of launches, and that the host hook ran (the list sort's plan was there)."""
import json
import os
import subprocess
import sys

import pytest

import sweep_recorded as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import vlg_matching_amd as v
    v.lib()
    return v


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "sweep_recorded.json")) as f:
        return json.load(f)["cases"]


def _compare(recorded, group, got):
    want = {name: obs for name, obs in recorded.items() if name.startswith(group + "/")}
    assert want and set(got) == set(want)
    for name, parts in want.items():
        assert set(got[name]) == set(parts), name
        for part, fields in parts.items():
            assert fields and {k: got[name][part][k] for k in fields} == fields, (name, part)


@pytest.mark.parametrize("group", [g for g in S.GROUPS if g not in S.GROUP_ENV])
def test_batches_leave_behind_what_was_recorded(V, recorded, group):
    _compare(recorded, group, {name: run() for name, run in S.cases(V, group).items()})


@pytest.mark.parametrize("group", list(S.GROUP_ENV))
def test_batches_of_a_fresh_process_leave_behind_what_was_recorded(recorded, group):
    """the groups whose environment the library reads: observed by the recorder's own --group run, in a process of its own"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "tools", "sweep_record.py"), "--group", group]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    _compare(recorded, group, json.loads(out.stdout.strip().splitlines()[-1]))
