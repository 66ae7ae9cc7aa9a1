"""No GPU: pipeline.heads_forward hands the kernels the same pointers, offsets, sizes, strides, scales and flags in the same
order, asks the workspace for the same buffers, and shows bench.py's stage profile the same launches, work and bytes as the
record in tests/golden/heads_launch_trace.json (tests/helpers/launch_trace.py: what is recorded, the seven configurations, and
how to regenerate the file).  Everything is compared with ==."""
import json
import os

import pytest

from tests.helpers import launch_trace


@pytest.fixture(scope="module")
def record():
    from mickey_amd import build
    if not os.path.exists(build.lib_path()):   # (ops.query stays real: mk_bordered_rows, mk_linattn_work_floats)
        build.build(verbose=False)
    with open(launch_trace.RECORD) as f:
        return json.load(f)


def test_the_record_holds_every_configuration(record):
    assert list(record) == list(launch_trace.CONFIGS)
    for rec in record.values():
        assert sorted(rec) == ["allocs", "calls", "profile"] and len(rec["calls"]) > 20


@pytest.mark.parametrize("name", list(launch_trace.CONFIGS))
def test_heads_forward_launches_what_the_record_holds(record, name):
    got = json.loads(json.dumps(launch_trace.trace(name)))   # (as the file holds it: lists, no tuples)
    for part in ("calls", "allocs", "profile"):
        assert got[part] == record[name][part], launch_trace.first_difference(part, got[part], record[name][part])
