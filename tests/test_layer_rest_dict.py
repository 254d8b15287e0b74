"""CPU tests of the tetrahedral rest dictionary of schedule LAYERED (PIES_LAYER_REST_SETS): the packing of the set index into the
spare bits of the tile-local node ids, the all-or-nothing rule, and which scenes take the dictionary, through host-only handles
(PIES_DEVICE_NONE)."""
import numpy as np
import pytest

import layer_rest_scenes
import scenes

CAP = 64  # kLayerRestMaxSets
LDS = 160 * 1024


def _host(pies, build, iterations=4):
    g = pies.Solver(scenes.pbd_options(pies, iterations), device=pies.DEVICE_NONE)
    build(g)
    g.set_flag(1, 0)
    g.set_schedule(pies.SCHEDULE_LAYERED)
    g.finalize()
    return g


def test_cap_is_the_bindings(pies):
    assert pies.LAYER_REST_MAX_SETS == CAP and pies.LAYER_REST_SETS == 23


@pytest.mark.parametrize("ids", [(0, 0, 0, 0), (8191, 8191, 8191, 8191), (8191, 0, 8191, 0), (1, 4097, 4096, 8190), (5461, 2730, 5461, 2730)])
@pytest.mark.parametrize("index", [0, 1, CAP - 1, 0o7070, 0o0707, 4095])
def test_pack_round_trip(pies, ids, index):
    words = pies.layer_rest_pack(ids, index)
    assert words is not None
    assert pies.layer_rest_unpack(words) == (list(ids), index)
    # the ids sit where the 16-bit ids sat, below 13 bits; the index fills exactly the 12 bits above them
    assert [words[0] & 0x1FFF, (words[0] >> 16) & 0x1FFF, words[1] & 0x1FFF, (words[1] >> 16) & 0x1FFF] == list(ids)
    assert pies.layer_rest_pack(ids, 0) == (ids[0] | ids[1] << 16, ids[2] | ids[3] << 16)


def test_pack_refuses_what_does_not_fit(pies):
    assert pies.layer_rest_pack((8192, 0, 0, 0), 0) is None
    assert pies.layer_rest_pack((0, 0, 0, 65535), 0) is None
    assert pies.layer_rest_pack((0, 0, 0, 0), 4096) is None


def test_all_or_nothing_rule(pies):
    ok = pies.layer_rest_usable
    assert ok(6, 1000, 800) and ok(CAP, 16 * CAP, 800) and ok(1, 16, 8)
    assert not ok(0, 1000, 800)
    assert not ok(CAP + 1, 100000, 800)           # more sets than the cap
    assert not ok(6, 95, 800) and ok(6, 96, 800)  # a real compression: sets * 16 <= elements
    assert not ok(6, 1000, 8193) and not ok(6, 1000, 9000)  # an id needs its 13 bits
    # table + node records (20 B each) + colour offsets (6 x 130 words) fit the LDS of a workgroup ...
    most = (LDS - 6 * 130 * 4 - 6 * 48) // 20
    assert ok(6, 1000, most) and not ok(6, 1000, most + 1)
    # ... and a launch that fitted a compute unit twice (the four-wavefronts-per-SIMD variants) still does
    half = (LDS // 2 - 6 * 130 * 4) // 20
    assert ok(6, 1000, half - 20) and not ok(6, 1000, half) and ok(6, 1000, half + 1)


def test_lattice_takes_the_dictionary_and_the_switch_turns_it_off(pies, tune):
    def build(s):
        scenes.build_beam(s, (4, 4, 12))
        scenes.perturb(s, 3, 0.05)  # positions move after the constraints exist: the rest data stay the lattice's
    g = _host(pies, build)
    n = g.count(pies.LAYER_REST_SETS)
    assert 0 < n <= 12, n
    assert n == len(np.unique(g.rest(pies.TET).view(np.uint32), axis=0))
    tune("PIES_LAYER_REST_DICT", "0")
    assert _host(pies, build).count(pies.LAYER_REST_SETS) == 0
    # another schedule has no dictionary
    tune("PIES_LAYER_REST_DICT", None)
    h = pies.Solver(scenes.pbd_options(pies, 4), device=pies.DEVICE_NONE)
    build(h)
    h.set_schedule(pies.SCHEDULE_COLOURED)
    h.finalize()
    assert h.count(pies.LAYER_REST_SETS) == 0


def test_sets_are_compared_by_bytes(pies):
    """-0.0 and +0.0 in a rest matrix are two sets; a changed w or strain limit is another set."""
    def base(s):
        scenes.build_beam(s, (4, 4, 12))
    g = _host(pies, base)
    n = g.count(pies.LAYER_REST_SETS)
    rest = g.rest(pies.TET)
    zeros = np.argwhere(rest.view(np.uint32) == 0)  # a +0.0 entry of some element's Qinv
    assert len(zeros)
    k, j = zeros[0]
    same = np.flatnonzero((rest.view(np.uint32) == rest.view(np.uint32)[k]).all(axis=1))
    assert len(same) > 1

    def negated(s):
        base(s)
        r = s.rest(pies.TET)[k:k + 1].copy()
        r[0, j] = np.float32(-0.0)
        s.set_rest(pies.TET, r, first=int(k))
    h = _host(pies, negated)
    assert np.signbit(h.rest(pies.TET)[k, j]) and h.rest(pies.TET)[k, j] == 0.0
    assert h.count(pies.LAYER_REST_SETS) == n + 1


def test_over_the_cap_falls_back(pies):
    """cap + 1 distinct w values over one lattice, through the constraint API: no dictionary (and no truncated index); cap / shapes
    values: the dictionary, with every (shape, w) set."""
    few = _host(pies, lambda s: layer_rest_scenes.lattice_with_w(s, 1))
    shapes = few.count(pies.LAYER_REST_SETS)
    assert 0 < shapes <= 12
    some = _host(pies, lambda s: layer_rest_scenes.lattice_with_w(s, 3))
    assert shapes < some.count(pies.LAYER_REST_SETS) <= 3 * shapes
    over = _host(pies, lambda s: layer_rest_scenes.lattice_with_w(s, CAP + 1))
    assert over.count(pies.TET) >= 16 * (CAP + 1)  # (not the compression rule)
    assert len(np.unique(over.rest(pies.TET).view(np.uint32), axis=0)) <= 12  # (w is no part of the rest matrix: the sets differ by w)
    assert over.count(pies.LAYER_REST_SETS) == 0


@pytest.mark.parametrize("name", sorted(layer_rest_scenes.CASES))
def test_gpu_cases_take_the_path_they_are_meant_to(pies, tune, name):
    """the scenes of tests/test_layer_rest_dict_gpu.py, on host-only handles"""
    case = layer_rest_scenes.CASES[name]
    for k, v in case.get("tuning", {}).items():
        tune(k, v)
    g = _host(pies, case["build"])
    n = g.count(pies.LAYER_REST_SETS)
    assert case["sets"](n), n


def test_every_element_distinct_has_no_dictionary(pies):
    mesh = scenes.delaunay_beam((4, 4, 10))
    g = _host(pies, lambda s: scenes.build_unstructured(s, mesh))
    assert g.count(pies.TET) > 0 and g.count(pies.LAYER_REST_SETS) == 0
