"""The substep sequencer (substep_graph.cpp) pinned scene by scene: launch counts after finalize and after the last tick, the CG
budget after every tick, the final state bit for bit, and what the two profile passes report, against the recording in
tests/golden/substep_sequence.json (tools/record_substep_sequence.py made it, twice, at the commit the file names; a state hash
the two recordings disagreed on is stored as null and not compared - none was)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("record_substep_sequence", os.path.join(ROOT, "tools", "record_substep_sequence.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(os.path.join(ROOT, "tests", "golden", "substep_sequence.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_scene_is_recorded_with_its_state():
    assert sorted(GOLDEN["scenes"]) == sorted(recorder.SCENES) and GOLDEN["parent_commit"]
    for name, rec in GOLDEN["scenes"].items():
        assert rec["state"] is not None or name.startswith(recorder.MAY_DROP_STATE), name
    assert "profile" in GOLDEN["scenes"]["04_layered_one_strip"] and "profile" in GOLDEN["scenes"]["10_pd_tiles_at_rest"]


@pytest.mark.parametrize("name", sorted(recorder.SCENES))
def test_sequence_equals_the_recording(pies, name):
    want = GOLDEN["scenes"][name]
    got = recorder.record_scene(pies, name)
    print(name, json.dumps(got, sort_keys=True))
    for key in ("launch_counts_finalize", "launch_counts_end", "budgets", "profile"):
        assert got.get(key) == want.get(key), (name, key, got.get(key), want.get(key))
    if want["state"] is not None:
        assert got["state"] == want["state"], (name, "state")
