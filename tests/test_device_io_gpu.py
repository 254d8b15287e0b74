"""GPU tests of pies_read_nodes_device / pies_write_nodes_device / pies_read_skin_device: node state and skins to and from device
memory of the caller.  Every comparison is bit for bit against the host paths (pies_read_nodes, pies_write_nodes,
pies_read_skin): the kernels copy words, so no tolerance applies.  The caller's memory is hipMalloc'ed through ctypes
(tests/device_buffers.py) with sentinels around every buffer."""
import ctypes as C

import numpy as np
import pytest

import scenes
from device_buffers import DevBuf, Hip
from test_node_renumber import shuffled_beam

pytestmark = pytest.mark.gpu
U = np.uint32
FIELDS = ("position", "prev_position", "velocity")
HOST = ("positions", "prev_positions", "velocities")
SETTERS = ("set_positions", "set_prev_positions", "set_velocities")
PBD_SCHEDULES = ("exact", "coloured", "layered")
CONFIGS = PBD_SCHEDULES + ("pd", "pd_renumbered")


@pytest.fixture(scope="module")
def hip():
    return Hip()


@pytest.fixture(scope="module")
def shuffled_mesh():
    return shuffled_beam()


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(U)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def loose(pies, n, seed=1):
    """n free nodes with their own velocities, radii and inverse masses (every fourth is fixed); no node-node pass"""
    rng = np.random.default_rng(seed + n)
    g = pies.Solver(scenes.pbd_options(pies, 2))
    inv = rng.uniform(0.5, 2.0, n).astype(np.float32)
    inv[::4] = 0.0
    g.add_nodes_raw(rng.uniform(1.0, 9.0, (n, 3)).astype(np.float32), vel=rng.uniform(-1, 1, (n, 3)).astype(np.float32),
                    radius=rng.uniform(0.1, 0.5, n).astype(np.float32), invMass=inv)
    g.set_flag(1, 0)
    return g


def beam(pies, config, mesh=None):
    """The 5 x 5 x 12 beam (300 nodes) under PBD in one of the three schedules or under PD; pd_renumbered: the shuffled Delaunay
    beam of tests/test_node_renumber_gpu.py with PIES_FLAG_RENUMBER_NODES"""
    if config == "pd_renumbered":
        from test_node_renumber_gpu import beam as shuffled_scene, renumbered
        g = renumbered(pies)
        shuffled_scene(g, mesh)
        g.finalize()
        assert g.count(pies.NODES_RENUMBERED) == 1
        return g
    if config == "pd":
        g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
        g.create_tet_box(5, 5, 12, translation=(0.0, 0.02, 0.0), w=1.0, volume=True, triangles=True)
        g.add_position(np.array([12 * (j + 5 * i) for i in range(5) for j in range(5)], dtype=U), 2.0)
        scenes.perturb(g, 9, 0.03)
        g.set_prev_positions(g.positions)
        return g
    g = pies.Solver(scenes.pbd_options(pies, 4))
    scenes.build_beam(g, (5, 5, 12))
    scenes.perturb(g, 1, 0.05)
    g.set_flag(1, 0)
    g.set_schedule({"exact": pies.SCHEDULE_EXACT, "coloured": pies.SCHEDULE_COLOURED, "layered": pies.SCHEDULE_LAYERED}[config])
    return g


def pin_budget(tune, config):
    if config.startswith("pd"):  # the host path synchronises more often: the captured CG budget must not follow that
        tune("PIES_PCG_BUDGET", "24")


def host_state(g):
    return [getattr(g, name) for name in HOST] + [g.radii, g.inv_masses]


def read_all(hip, g, stride, offset=0, stream=0, flags=0):
    """all five arrays in one call; returns them as the host getters shape them (stride 4: the fourth column is checked to be 0)"""
    n = g.count(9)
    bufs = [DevBuf(hip, stride * n, offset) for _ in range(3)] + [DevBuf(hip, n, offset) for _ in range(2)]
    g.read_nodes_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, stride=stride, stream=stream, flags=flags)
    out = []
    for k, b in enumerate(bufs):
        a = b.get().copy()
        if k < 3:
            a = a.reshape(n, stride)
            if stride == 4:
                assert not bits(a[:, 3]).any(), "the fourth float must be +0.0"
            a = a[:, :3]
        out.append(a)
        b.free()
    return out


def check_reads(hip, g):
    want = host_state(g)
    for stride in (3, 4):
        for offset in (0, 1):
            got = read_all(hip, g, stride, offset)
            for name, a, b in zip(HOST + ("radii", "inv_masses"), got, want):
                assert same(a, b), (name, stride, offset)
    # one array at a time is the same launch with four arrays left out
    n = g.count(9)
    for k, field in enumerate(FIELDS):
        b = DevBuf(hip, 3 * n)
        g.read_nodes_device(**{field: b.ptr})
        assert same(b.get(), want[k]), field
        b.free()
    for k, field in ((3, "radius"), (4, "inv_mass")):
        b = DevBuf(hip, n, 1)
        g.read_nodes_device(**{field: b.ptr})
        assert same(b.get(), want[k]), field
        b.free()


# ---- reads -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "staged"])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257])
def test_reads_of_loose_nodes(pies, hip, tune, n, variant):
    """tile edges (255, 256, 257) and row counts whose 3 n floats are no multiple of four"""
    tune("PIES_NODE_IO_VARIANT", variant)
    g = loose(pies, n)
    check_reads(hip, g)  # before any tick: the scene is brought to the device by the call itself
    g.tick()
    check_reads(hip, g)
    g.close()


@pytest.mark.parametrize("variant", ["plain", "staged"])
@pytest.mark.parametrize("config", CONFIGS)
def test_reads_of_a_ticked_body(pies, hip, tune, shuffled_mesh, config, variant):
    tune("PIES_NODE_IO_VARIANT", variant)
    g = beam(pies, config, shuffled_mesh)
    g.tick(3)
    assert not g.failed
    check_reads(hip, g)
    g.close()


def test_default_variant_is_one_of_the_two(pies, hip, tune):
    g = loose(pies, 257)
    a = read_all(hip, g, 3)
    for variant in ("plain", "staged"):
        tune("PIES_NODE_IO_VARIANT", variant)
        b = read_all(hip, g, 3)
        assert all(same(x, y) for x, y in zip(a, b))
    g.close()


@pytest.mark.parametrize("config", ["layered", "pd"])
def test_reads_change_nothing(pies, hip, tune, config):
    """ten ticks with a read after each = ten ticks without"""
    pin_budget(tune, config)
    with_reads, without = beam(pies, config), beam(pies, config)
    n = with_reads.count(9)
    bufs = [DevBuf(hip, 4 * n) for _ in range(3)] + [DevBuf(hip, n) for _ in range(2)]
    for _ in range(10):
        with_reads.tick_async()
        with_reads.read_nodes_device(*[b.ptr for b in bufs], stride=4)
        without.tick_async()
    a, b = host_state(with_reads), host_state(without)
    assert all(same(x, y) for x, y in zip(a, b))
    assert same(bufs[0].get().reshape(n, 4)[:, :3], a[0])
    for buf in bufs:
        buf.free()
    with_reads.close()
    without.close()


# ---- writes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
def test_device_write_equals_host_write(pies, hip, tune, shuffled_mesh, config):
    """two handles, the same scene and 2 ticks; each of the three arrays in turn is replaced through pies_write_nodes on one and
    through pies_write_nodes_device on the other; after 3 more ticks the node state is identical"""
    pin_budget(tune, config)
    for k in range(3):
        host, dev = beam(pies, config, shuffled_mesh), beam(pies, config, shuffled_mesh)
        host.tick(2)
        dev.tick(2)
        n = host.count(9)
        rng = np.random.default_rng(40 + k)
        if k == 2:
            new = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
        else:
            new = getattr(host, HOST[k]) + rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32)
        getattr(host, SETTERS[k])(new)
        stride, variant = (3, "staged") if k == 1 else (4, "plain") if k == 0 else (3, "plain")
        tune("PIES_NODE_IO_VARIANT", variant)
        rows = new if stride == 3 else np.concatenate([new, np.full((n, 1), np.float32(777.0))], axis=1)
        src = DevBuf(hip, stride * n, offset=k % 2, fill=rows)
        dev.write_nodes_device(stride=stride, **{FIELDS[k]: src.ptr})
        assert same(src.get(), rows)  # the source is read only
        host.tick(3)
        dev.tick(3)
        assert not host.failed and not dev.failed
        for name in HOST + ("inv_masses",):
            assert same(getattr(host, name), getattr(dev, name)), (config, FIELDS[k], name)
        src.free()
        host.close()
        dev.close()


def test_position_write_keeps_the_mass(pies, hip):
    """stride 4 with junk in the source's fourth float: the next export frame's fourth float is still the inverse mass"""
    g = loose(pies, 257)
    g.tick()
    n, inv = 257, g.inv_masses
    assert (inv == 0).any() and (inv > 0).any()
    rows = np.concatenate([g.positions + np.float32(0.25), np.full((n, 1), np.float32(-3.5e9))], axis=1).astype(np.float32)
    src = DevBuf(hip, 4 * n, fill=rows)
    g.write_nodes_device(position=src.ptr, stride=4)
    got = read_all(hip, g, 4)
    assert same(got[0], rows[:, :3]) and same(got[4], inv)
    f = g.tick_begin()
    frame = g.export_acquire(f).copy()
    g.export_release(f)
    assert same(frame[:, 3], inv)
    assert same(g.inv_masses, inv) and same(frame[:, :3], g.positions)
    src.free()
    g.close()


@pytest.mark.parametrize("config", ["layered", "pd_renumbered"])
def test_indexed_writes(pies, hip, shuffled_mesh, config):
    """seven distinct ids with 0 and n - 1 among them and one id >= n: those seven rows change, every other word stays"""
    g = beam(pies, config, shuffled_mesh)
    g.tick()
    n = g.count(9)
    ids = np.array([0, n - 1, 5, n + 3, 17, 100, 255, 256], U)
    live = ids < n
    rng = np.random.default_rng(8)
    for k, field in enumerate(FIELDS):
        for stride in (3, 4):
            before = host_state(g)
            rows = rng.uniform(-2, 2, (len(ids), stride)).astype(np.float32)
            src, idb = DevBuf(hip, rows.size, fill=rows), DevBuf(hip, len(ids), offset=1, fill=ids.view(np.float32))
            g.write_nodes_device(stride=stride, ids=idb.ptr, m=len(ids), **{field: src.ptr})
            want = [a.copy() for a in before]
            want[k][ids[live]] = rows[live, :3]
            for via in (read_all(hip, g, 3), host_state(g)):
                for name, a, b in zip(HOST + ("radii", "inv_masses"), via, want):
                    assert same(a, b), (field, stride, name)
            assert same(src.get(), rows) and np.array_equal(idb.get(U), ids)
            src.free()
            idb.free()
    g.tick()
    assert not g.failed
    g.close()


def test_call_order(pies, hip):
    """a host write, then a device write: both reads show both edits; an appended body changes the n the calls accept"""
    g = beam(pies, "layered")
    g.tick(2)
    n = g.count(9)
    p1 = g.positions + np.float32(0.125)
    v1 = np.random.default_rng(2).uniform(-1, 1, (n, 3)).astype(np.float32)
    g.set_positions(p1)  # pending in the host mirror
    src = DevBuf(hip, 3 * n, fill=v1)
    g.write_nodes_device(velocity=src.ptr)  # uploads the mirror first, then scatters
    dev = read_all(hip, g, 3)
    assert same(dev[0], p1) and same(dev[2], v1)
    assert same(g.positions, p1) and same(g.velocities, v1)
    # a later host write sees the scatter's result as well
    g.set_prev_positions(p1)
    dev = read_all(hip, g, 4, 1)
    assert same(dev[0], p1) and same(dev[1], p1) and same(dev[2], v1)
    g.create_tet_box(3, 3, 3, translation=(20.0, 5.0, 0.0), w=0.05)
    n2 = g.count(9)
    assert n2 == n + 27
    a = pies.DeviceNodes(velocity=src.ptr, stride=3)
    L = pies.load()
    assert L.pies_read_nodes_device(g._h, C.byref(a), n, None, 0) == pies.ERR_INVALID
    assert L.pies_write_nodes_device(g._h, C.byref(a), None, n, None, 0) == pies.ERR_INVALID
    dev = read_all(hip, g, 3)
    assert len(dev[0]) == n2 and same(dev[0][:n], p1) and same(dev[2][:n], v1) and same(dev[0], g.positions)
    src.free()
    g.close()


def test_invalid_device_pointers(pies, hip):
    """host memory, and an array that runs past its allocation, are refused before anything is launched"""
    g = loose(pies, 64)
    host = np.zeros(3 * 64, np.float32)
    L = pies.load()
    a = pies.DeviceNodes(position=host.ctypes.data, stride=3)
    assert L.pies_read_nodes_device(g._h, C.byref(a), 64, None, 0) == pies.ERR_INVALID
    assert L.pies_write_nodes_device(g._h, C.byref(a), None, 64, None, 0) == pies.ERR_INVALID
    small = DevBuf(hip, 3 * 64 - 16)
    a = pies.DeviceNodes(position=small.ptr, stride=3)
    assert L.pies_read_nodes_device(g._h, C.byref(a), 64, None, 0) == pies.ERR_INVALID
    assert "allocation" in g.last_error()
    small.get()
    ok = DevBuf(hip, 3 * 64)
    g.read_nodes_device(position=ok.ptr, flags=pies.IO_HOST_SYNC)  # the handle still works
    assert same(ok.get(), g.positions)
    small.free()
    ok.free()
    g.close()


def test_frames_in_flight(pies, hip):
    """tick_begin, a device write, export_acquire: the frame holds the state before the write, the device the state after it"""
    g, twin = beam(pies, "layered"), beam(pies, "layered")
    n = g.count(9)
    f = g.tick_begin()
    new = np.random.default_rng(3).uniform(1.0, 6.0, (n, 3)).astype(np.float32)
    src = DevBuf(hip, 3 * n, fill=new)
    g.write_nodes_device(position=src.ptr)
    frame = g.export_acquire(f).copy()
    g.export_release(f)
    twin.tick()
    assert same(frame[:, :3], twin.positions)
    assert same(g.positions, new) and same(read_all(hip, g, 3)[0], new)
    src.free()
    g.close()
    twin.close()


def test_stream_order(pies, hip):
    """on a stream of the caller's: a memset of the destination, the read, a copy out, ONE synchronisation - the copy holds the
    node state, so the read ran behind the memset and before the copy"""
    g = beam(pies, "layered")
    g.tick(2)
    n = g.count(9)
    L = hip.L
    stream, pinned = C.c_void_p(), C.c_void_p()
    hip.ok(L.hipStreamCreate(C.byref(stream)))
    hip.ok(L.hipHostMalloc(C.byref(pinned), 12 * n, 0))
    out = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_float)), shape=(3 * n,))
    out[:] = -1.0
    dst = DevBuf(hip, 3 * n)
    g.tick_async()  # queued work in front of the read on the solver's stream
    g.synchronize()
    want = g.velocities
    hip.ok(L.hipMemsetAsync(dst.ptr, 0x7F, 12 * n, stream))
    g.read_nodes_device(velocity=dst.ptr, stream=stream.value)
    hip.ok(L.hipMemcpyAsync(pinned, dst.ptr, 12 * n, 2, stream))
    hip.ok(L.hipStreamSynchronize(stream))
    assert same(out, want)
    dst.get()
    hip.ok(L.hipHostFree(pinned))
    hip.ok(L.hipStreamDestroy(stream))
    dst.free()
    g.close()


# ---- skins -----------------------------------------------------------------------------------------------------------------------
def test_skins(pies, hip):
    """pies_read_skin_device = pies_read_skin for two skins, with and without normals"""
    from test_skin import T0, lattice, skin_mesh
    g = pies.Solver(pies.Options(solver=pies.PD, iterations=10))
    tets = lattice(g)
    lo, hi = np.float32(T0) + 0.05, np.float32(T0) + 1.95
    v, tri = skin_mesh(257, lo, hi)
    g.add_skin(v, tets, tri)
    t2 = np.float32([5.25, 1.5, 0.5])
    tets2 = lattice(g, translation=tuple(t2))
    v2, tri2 = skin_mesh(63, t2 + 0.05, t2 + 1.95)
    g.add_skin(v2, tets2, tri2)
    scenes.perturb(g, 6, 0.04)
    g.set_prev_positions(g.positions)
    g.tick(2)
    for skin, count in ((0, 257), (1, 63)):
        x, nr = g.read_skin(skin)
        assert len(x) == count and np.abs(nr).max() > 0.5
        for offset in (0, 1):
            px, pn = DevBuf(hip, 3 * count, offset), DevBuf(hip, 3 * count, offset)
            g.read_skin_device(skin, px.ptr, pn.ptr)
            assert same(px.get(), x) and same(pn.get(), nr)
            px.free()
            pn.free()
        px = DevBuf(hip, 3 * count)
        g.read_skin_device(skin, px.ptr)  # normals = NULL
        assert same(px.get(), x)
        px.free()
    g.close()
