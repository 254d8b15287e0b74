"""pies_read_nodes_device / pies_write_nodes_device / pies_read_skin_device on a host-only handle (PIES_DEVICE_NONE): the argument
checks come first - every invalid argument is PIES_ERR_INVALID, a radius or inverse-mass write PIES_ERR_UNSUPPORTED - and a
well-formed call then fails with PIES_ERR_HIP, because the node state lives on a device.  No GPU is needed: the pointers are
never followed (whether they are device memory is checked after the handle's device, which this handle does not have)."""
import ctypes as C

import numpy as np
import pytest

from pies_amd import capi

ADDR = 0x7F0000001000  # 16-byte aligned; never dereferenced on a host-only handle


@pytest.fixture
def g():
    s = capi.Solver(capi.Options(solver=capi.PBD, iterations=2), device=capi.DEVICE_NONE)
    s.addNodes(np.arange(15, dtype=np.float32).reshape(5, 3))
    yield s
    s.close()


@pytest.fixture
def skinned():
    s = capi.Solver(capi.Options(solver=capi.PBD, iterations=2), device=capi.DEVICE_NONE)
    s.create_tet_box(2, 2, 2, w=1.0)
    tets = s.ids(capi.TET).reshape(-1, 4)
    s.add_skin(s.positions[tets[0]].mean(0, keepdims=True), tets, None, 0.0)
    yield s
    s.close()


def nodes(stride=3, **kw):
    return capi.DeviceNodes(stride=stride, **kw)


def read(g, a, n=5, stream=None, flags=0):
    return capi.load().pies_read_nodes_device(g._h, C.byref(a) if a is not None else None, n, stream, flags)


def write(g, a, m=5, ids=None, stream=None, flags=0):
    return capi.load().pies_write_nodes_device(g._h, C.byref(a) if a is not None else None, ids, m, stream, flags)


def test_symbols_and_flag():
    L = capi.load()
    assert all(hasattr(L, name) for name in ("pies_read_nodes_device", "pies_write_nodes_device", "pies_read_skin_device"))
    assert capi.IO_HOST_SYNC == 1 and L.pies_abi_version() == 4
    assert C.sizeof(capi.DeviceNodes) == 5 * C.sizeof(C.c_void_p) + 8  # five pointers, the stride, padding


def test_null_handle_and_struct(g):
    L = capi.load()
    a = nodes(position=ADDR)
    assert L.pies_read_nodes_device(None, C.byref(a), 5, None, 0) == capi.ERR_INVALID
    assert L.pies_write_nodes_device(None, C.byref(a), None, 5, None, 0) == capi.ERR_INVALID
    assert L.pies_read_skin_device(None, 0, ADDR, None, 1, None, 0) == capi.ERR_INVALID
    assert read(g, None) == capi.ERR_INVALID and write(g, None) == capi.ERR_INVALID


@pytest.mark.parametrize("call", [read, write])
def test_invalid_node_arguments(g, call):
    assert call(g, nodes()) == capi.ERR_INVALID  # every pointer NULL
    assert "NULL" in g.last_error()
    for stride in (0, 1, 2, 5, 12):
        assert call(g, nodes(stride=stride, position=ADDR)) == capi.ERR_INVALID
    assert "stride" in g.last_error()
    for count in (0, 4, 6):  # a wrong n (m with ids == NULL)
        assert call(g, nodes(position=ADDR), count) == capi.ERR_INVALID
    assert "node count" in g.last_error()
    for field in ("position", "prev_position", "velocity"):
        for off in (1, 2, 3):
            assert call(g, nodes(**{field: ADDR + off})) == capi.ERR_INVALID
        assert "aligned" in g.last_error()
        assert call(g, nodes(**{field: ADDR + 4})) == capi.ERR_HIP  # one float off a 16-byte boundary is fine


def test_invalid_read_only_arrays(g):
    for field in ("radius", "inv_mass"):
        assert read(g, nodes(**{field: ADDR + 2})) == capi.ERR_INVALID
        assert read(g, nodes(**{field: ADDR + 4})) == capi.ERR_HIP
        assert write(g, nodes(**{field: ADDR})) == capi.ERR_UNSUPPORTED
        assert write(g, nodes(velocity=ADDR, **{field: ADDR + 64})) == capi.ERR_UNSUPPORTED
        assert "pies_write_nodes" in g.last_error()


def test_indexed_write_arguments(g):
    ids = C.c_void_p(ADDR + 4096)
    assert write(g, nodes(velocity=ADDR), 3, ids) == capi.ERR_HIP  # any m with ids
    assert write(g, nodes(velocity=ADDR), 9, ids) == capi.ERR_HIP
    assert write(g, nodes(velocity=ADDR), 0, ids) == capi.OK
    assert write(g, nodes(velocity=ADDR), 3, C.c_void_p(ADDR + 4098)) == capi.ERR_INVALID
    assert write(g, nodes(), 3, ids) == capi.ERR_INVALID


def test_well_formed_calls_need_a_device(g):
    for stride in (3, 4):
        assert read(g, nodes(stride, position=ADDR, prev_position=ADDR + 256, velocity=ADDR + 512, radius=ADDR + 768,
                             inv_mass=ADDR + 1024)) == capi.ERR_HIP
        assert "PIES_DEVICE_NONE" in g.last_error()
        assert read(g, nodes(stride, inv_mass=ADDR), flags=capi.IO_HOST_SYNC) == capi.ERR_HIP
        assert write(g, nodes(stride, position=ADDR, prev_position=ADDR + 256, velocity=ADDR + 512)) == capi.ERR_HIP
        assert "PIES_DEVICE_NONE" in g.last_error()
    with pytest.raises(capi.PiesError):
        g.read_nodes_device(position=ADDR)
    with pytest.raises(capi.PiesError):
        g.write_nodes_device(velocity=ADDR, stride=4)


def test_empty_scene_is_ok():
    s = capi.Solver(capi.Options(solver=capi.PBD), device=capi.DEVICE_NONE)
    assert read(s, nodes(position=ADDR), 0) == capi.OK and write(s, nodes(position=ADDR), 0) == capi.OK
    assert read(s, nodes(position=ADDR), 1) == capi.ERR_INVALID
    assert read(s, nodes(), 0) == capi.ERR_INVALID  # the arguments are still checked
    s.close()


def test_variant_switch_is_checked(g, tune):
    for value in ("plain", "staged"):
        tune("PIES_NODE_IO_VARIANT", value)
        assert read(g, nodes(position=ADDR)) == capi.ERR_HIP and write(g, nodes(position=ADDR)) == capi.ERR_HIP
    tune("PIES_NODE_IO_VARIANT", "wide")
    assert read(g, nodes(position=ADDR)) == capi.ERR_INVALID and write(g, nodes(position=ADDR)) == capi.ERR_INVALID
    assert "PIES_NODE_IO_VARIANT" in g.last_error()


def test_skin_arguments(skinned):
    L, h = capi.load(), skinned._h
    assert skinned.skin_vertex_count(0) == 1
    assert L.pies_read_skin_device(h, 1, ADDR, None, 1, None, 0) == capi.ERR_INVALID  # an unknown skin
    assert L.pies_read_skin_device(h, 0, None, ADDR, 1, None, 0) == capi.ERR_INVALID  # positions are not optional
    assert L.pies_read_skin_device(h, 0, ADDR, None, 2, None, 0) == capi.ERR_INVALID  # a wrong n
    assert L.pies_read_skin_device(h, 0, ADDR + 2, None, 1, None, 0) == capi.ERR_INVALID
    assert L.pies_read_skin_device(h, 0, ADDR, ADDR + 65, 1, None, 0) == capi.ERR_INVALID
    assert L.pies_read_skin_device(h, 0, ADDR, None, 1, None, 0) == capi.ERR_HIP
    assert L.pies_read_skin_device(h, 0, ADDR, ADDR + 64, 1, None, capi.IO_HOST_SYNC) == capi.ERR_HIP
    with pytest.raises(capi.PiesError):
        skinned.read_skin_device(0, ADDR)
