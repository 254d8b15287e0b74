"""One handle taken through unlike scenes: everything a pies_finalize built is taken down by free_device (pies_clear, a change of
solver or schedule) before the next one builds its own, so no stage may see a buffer, a count or a flag of the stage before it.

Stages, in order, on one handle:
  (a) PBD, schedule LAYERED, a 6 x 6 x 12 beam with node-node collisions, 2 ticks;
  (b) clear(), then PD: a 4 x 4 x 10 beam with volume constraints, triangles and a pinned end cap, PIES_FLAG_PD_NODE_CONTACTS and
      one listed node pair, 2 ticks;
  (c) the same scene as it then stands under PBD with schedule EXACT, 1 tick;
  (d) clear(), then scene (a) again, 2 ticks.
After every stage the positions and velocities equal, bit for bit, those of a fresh handle given that stage's scene and ticks
alone - the PD stage too: the CG budget it starts from is the same on both handles.  The launch counts are not compared: the
adapted counts (level launches of the pair order, sort passes, the CG budget) carry over from stage to stage by design."""
import numpy as np
import pytest

import scenes
from test_pd_parity_gpu import build_pd_beam

pytestmark = pytest.mark.gpu


def options(pies):
    return pies.Options(solver=pies.PBD, iterations=4, timeSubsteps=1, fixedTimestepSize=0.012, gravity=10.0, floorHeight=0.0)


def scene_a(pies, s):
    s.set_solver(pies.PBD)
    s.set_schedule(pies.SCHEDULE_LAYERED)
    s.set_flag(pies.FLAG_NODE_COLLISIONS, 1)
    s.set_flag(pies.FLAG_PD_NODE_CONTACTS, 0)
    scenes.build_beam(s, (6, 6, 12))
    scenes.perturb(s, 21, 0.05)
    s.set_prev_positions(s.positions)


def scene_b(pies, s):
    s.set_solver(pies.PD)
    s.set_flag(pies.FLAG_PD_NODE_CONTACTS, 1)
    build_pd_beam(s, (4, 4, 10))
    s.add_node_pairs(np.uint32([[3, 157]]))  # two nodes that share no element
    scenes.perturb(s, 22, 0.04)
    s.set_prev_positions(s.positions)


def same_state(stage, reused, fresh):
    for name in ("positions", "velocities"):
        a, b = getattr(reused, name), getattr(fresh, name)
        assert np.isfinite(b).all(), (stage, name)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
            (stage, name, "max |reused - fresh| = %.3g" % float(np.abs(a - b).max()))


def test_one_handle_through_unlike_scenes(pies):
    h = pies.Solver(options(pies))

    scene_a(pies, h)
    h.tick(2)
    fresh_a = pies.Solver(options(pies))
    scene_a(pies, fresh_a)
    fresh_a.tick(2)
    assert fresh_a.launch_counts()["layer"] > 0  # schedule LAYERED took the scene
    same_state("a", h, fresh_a)

    h.clear()
    scene_b(pies, h)
    h.tick(2)
    f = pies.Solver(options(pies))
    scene_b(pies, f)
    assert f.count(pies.NODE_PAIRS) == 1 and f.count(pies.VOLUME) == f.count(pies.TET) > 0 and f.count(pies.TRIANGLES) > 0
    f.tick(2)
    same_state("b", h, f)

    # (c): the fresh handle gets scene (b) in the state stage (b) left it in, as a PBD scene from the start
    pos, prev, vel = h.positions, h.prev_positions, h.velocities
    h.set_solver(pies.PBD)
    h.set_schedule(pies.SCHEDULE_EXACT)
    h.tick(1)
    f = pies.Solver(options(pies))
    scene_b(pies, f)
    f.set_solver(pies.PBD)
    f.set_schedule(pies.SCHEDULE_EXACT)
    f.set_positions(pos)
    f.set_prev_positions(prev)
    f.set_velocities(vel)
    f.tick(1)
    assert not np.array_equal(f.positions, pos)
    same_state("c", h, f)

    h.clear()
    scene_a(pies, h)
    h.tick(2)
    same_state("d", h, fresh_a)
