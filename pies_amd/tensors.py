"""Node state and skins of a pies_amd.capi.Solver as torch tensors on the solver's device (pies_read_nodes_device /
pies_write_nodes_device / pies_read_skin_device): nothing crosses the bus and nothing here synchronises the host.

    import torch                                   # (this module imports it first too)
    from pies_amd import capi, tensors
    g = capi.Solver(...); ...; io = tensors.Tensors(g)
    g.tick_async(); x = io.positions(); io.set_velocities((x[ids] - target) * -k, ids)

The calls are ordered against torch.cuda.current_stream(device): work queued on it before a call is finished before the
library touches the tensors, work queued after it sees the result.

torch ships a HIP runtime of its own under the same SONAME as the system's.  Imported first, it is the runtime the loader
gives libpies_hip.so as well, and streams, events and allocations are one world.  With libpies_hip.so loaded first the process
ends up with two runtimes whose handles mean nothing to each other: this module imports torch before it loads the library and
Tensors() refuses to work in a process where two different libamdhip64 files are mapped.  `import pies_amd` alone still does
not need torch.
"""
import os

import torch  # before capi.load(): see above

from . import capi


def hip_runtimes():
    """The distinct libamdhip64 files mapped into this process (real paths)."""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                parts = line.split(None, 5)
                path = parts[5].strip() if len(parts) == 6 else ""
                if "libamdhip64" in os.path.basename(path):
                    found.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(found)


def check_single_runtime():
    libs = hip_runtimes()
    if len(libs) > 1:
        raise capi.PiesError("two HIP runtimes are mapped (%s): libpies_hip.so was loaded before torch, so its streams and "
                             "allocations are not torch's.  Import torch (or pies_amd.tensors) before anything calls "
                             "pies_amd.capi.load()" % ", ".join(libs))
    return libs


class Tensors:
    """Tensor access to one solver.  Getters return float32 tensors in host numbering, (n, 3) or with stride=4 (n, 4) with a
    fourth column of zeros; `out=` reuses a tensor of that shape.  Setters take (n, 3) or (n, 4) tensors (a fourth column is
    ignored), or with ids (m, 3|4) rows for the listed nodes."""

    def __init__(self, solver, device=None):
        capi.load()
        check_single_runtime()
        self.solver = solver
        if device is None:
            device = solver.device
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)

    # -- helpers ---------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _n(self):
        return self.solver.count(capi.NODES)

    def _out(self, out, shape):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if out.requires_grad:
            raise capi.PiesError("out= tensor requires grad: the library writes it in place, outside autograd")
        if out.dtype != torch.float32 or out.device != self.device or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
            raise capi.PiesError("out= must be a contiguous float32 tensor of shape %s on %s" % (tuple(shape), self.device))
        return out

    def _rows(self, t, m):
        if not isinstance(t, torch.Tensor):
            raise capi.PiesError("a torch tensor is expected")
        if t.device != self.device:
            raise capi.PiesError("the tensor is on %s, the solver on %s" % (t.device, self.device))
        if t.dim() != 2 or t.shape[0] != m or t.shape[1] not in (3, 4):
            raise capi.PiesError("expected a (%d, 3) or (%d, 4) tensor, got %s" % (m, m, tuple(t.shape)))
        return t.detach().to(torch.float32).contiguous()

    def _read_vec(self, field, out, stride):
        if stride is None:  # the out= tensor decides, else the packed form
            stride = out.shape[1] if out is not None and out.dim() == 2 and out.shape[1] in (3, 4) else 3
        out = self._out(out, (self._n(), stride))
        if out.shape[0]:
            self.solver.read_nodes_device(stride=stride, stream=self._stream(), **{field: out.data_ptr()})
        return out

    def _read_scalar(self, field, out):
        out = self._out(out, (self._n(),))
        if out.shape[0]:
            self.solver.read_nodes_device(stream=self._stream(), **{field: out.data_ptr()})
        return out

    def _write(self, field, t, ids):
        n = self._n()
        if ids is None:
            t = self._rows(t, n)
            if n:
                self.solver.write_nodes_device(stride=t.shape[1], stream=self._stream(), **{field: t.data_ptr()})
            return
        if not isinstance(ids, torch.Tensor) or ids.device != self.device or ids.dim() != 1:
            raise capi.PiesError("ids must be a 1-d integer tensor on %s" % self.device)
        if ids.dtype not in (torch.int32, torch.uint32):
            if ids.dtype not in (torch.int64, torch.int16, torch.uint8, torch.int8):
                raise capi.PiesError("ids must be an integer tensor")
            ids = ids.to(torch.int32)  # on the device
        ids = ids.contiguous()
        t = self._rows(t, ids.shape[0])
        if ids.shape[0]:
            self.solver.write_nodes_device(stride=t.shape[1], ids=ids.data_ptr(), m=ids.shape[0], stream=self._stream(),
                                           **{field: t.data_ptr()})
        # (ids and t stay alive until the launch is queued; the caching allocator keeps their memory for the stream's later work)

    # -- reads -----------------------------------------------------------------------------------
    def positions(self, out=None, stride=None):
        return self._read_vec("position", out, stride)

    def prev_positions(self, out=None, stride=None):
        return self._read_vec("prev_position", out, stride)

    def velocities(self, out=None, stride=None):
        return self._read_vec("velocity", out, stride)

    def radii(self, out=None):
        return self._read_scalar("radius", out)

    def inv_masses(self, out=None):
        return self._read_scalar("inv_mass", out)

    def state(self, positions=None, velocities=None, stride=3):
        """(positions, velocities) in one call: one launch"""
        n = self._n()
        x, v = self._out(positions, (n, stride)), self._out(velocities, (n, stride))
        if n:
            self.solver.read_nodes_device(position=x.data_ptr(), velocity=v.data_ptr(), stride=stride, stream=self._stream())
        return x, v

    # -- writes ----------------------------------------------------------------------------------
    def set_positions(self, t, ids=None):
        self._write("position", t, ids)

    def set_prev_positions(self, t, ids=None):
        self._write("prev_position", t, ids)

    def set_velocities(self, t, ids=None):
        self._write("velocity", t, ids)

    # -- actuators -------------------------------------------------------------------------------
    def _words(self, t, shape, dtypes, name):
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype not in dtypes or tuple(t.shape) != tuple(shape) \
                or not t.is_contiguous() or t.requires_grad:
            raise capi.PiesError("%s must be a contiguous %s tensor of shape %s on %s that does not require grad"
                                 % (name, " or ".join(str(d) for d in dtypes), tuple(shape), self.device))
        return t.data_ptr()

    def drive_actuators(self, actuator_set, activation, sums=None, live=None, per_actuator=None):
        """pies_drive_actuators_device: the set's rest lengths and angles written from `activation`, a float32 tensor with one
        entry per channel of the set - the output of a policy, say - without the host in the loop.  The optional outputs are
        tensors the library fills: sums float32 (c, 2), live int32 or uint32 (c), per_actuator float32 (n, 2).  A non-finite
        activation leaves its actuators' constraints as they are (the call cannot check the tensor)."""
        if not isinstance(activation, torch.Tensor) or activation.device != self.device or activation.dim() != 1:
            raise capi.PiesError("activation must be a 1-d tensor on %s" % (self.device,))
        u = activation.detach().to(torch.float32).contiguous()
        c = u.shape[0]
        n = len(self.solver.get_actuators(actuator_set)[0]) if per_actuator is not None else 0
        self.solver.drive_actuators_device(actuator_set, c, u.data_ptr(),
                                           sums=self._words(sums, (c, 2), (torch.float32,), "sums"),
                                           live=self._words(live, (c,), (torch.int32, torch.uint32), "live"),
                                           per_actuator=self._words(per_actuator, (n, 2), (torch.float32,), "per_actuator"),
                                           stream=self._stream())
        # (u stays alive until the launch is queued; the caching allocator keeps its memory for the stream's later work)

    # -- skins -----------------------------------------------------------------------------------
    def skin(self, k, normals=True):
        """(positions, normals) of skin k as (n, 3) tensors, or the positions alone with normals=False"""
        n = self.solver.skin_vertex_count(k)
        x = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        nr = torch.empty((n, 3), dtype=torch.float32, device=self.device) if normals else None
        if n:
            self.solver.read_skin_device(k, x.data_ptr(), nr.data_ptr() if normals else 0, n=n, stream=self._stream())
        return (x, nr) if normals else x
