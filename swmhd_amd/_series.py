"""What the device diagnostics (output, derived, zonal, spectra, spectra2d) share on the host side, stated once: how a list of names
is cut into launches, where the state of a model is, the allocate-or-check of a result tensor, the cached workspace, and the writer
that collects samples in one device tensor for swmhd_amd.output.run()."""
import torch

from . import _lib


def cut_runs(names, bits, tracers, messages):
    """`names` as launches: a kernel writes the fields of a mask in bit order, so the names are cut into runs of bits (from `bits`,
    name -> bit) that ascend in that order -- one launch for any ascending list, and any order or repetition of names is honoured.
    messages: the SwmhdError texts (for a tracer, for an unknown name -- both formatted with n -- and for no names at all)."""
    tracer, unknown, empty = messages
    runs = []
    for n in names:
        if n in tracers:
            raise _lib.SwmhdError(tracer.format(n=n))
        if n not in bits:
            raise _lib.SwmhdError(unknown.format(n=n))
        bit = bits[n]
        if runs and bit > runs[-1][-1]:
            runs[-1].append(bit)
        else:
            runs.append([bit])
    if not runs:
        raise _lib.SwmhdError(empty)
    return runs


def lead_shape(model):
    """() of one grid, (members,) of an ensemble: what a result's shape starts with"""
    members = getattr(model, "members", None)
    return (members,) if members is not None else ()


def state_device(model):
    return model._state[0].device if getattr(model, "members", None) is not None else model._raw_fields[0].data.device


def state_pointers(model):
    """(the four parents' device pointers, row stride, device, is an ensemble) of the state as it stands now"""
    if getattr(model, "members", None) is not None:
        q = model._state                  # (whichever set of tensors is the state NOW: the ping-pong roles flip every stage)
        return [t.data_ptr() for t in q], q[0].stride(1), q[0].device, True
    model._join()                         # a ring exchange of this state may still be in flight
    q = model._raw_fields
    return [f.ptr for f in q], q[0].stride_y, q[0].data.device, False


def out_tensor(out, shape, dtypes, dev, what, axis_word, array_type=None, row_stride=0):
    """The result tensor of an enqueue call: allocated (out is None; array_type, one of `dtypes`, or the first of them), or the
    caller's, checked: on the device, of `dtypes` and `shape`, unit stride in its last axis and at least row_stride in the one before."""
    if out is None:
        if array_type is None:
            array_type = dtypes[0]
        if array_type not in dtypes:
            raise _lib.SwmhdError(f"array_type {array_type}: {' or '.join(str(d) for d in dtypes)}")
        return torch.empty(shape, dtype=array_type, device=dev)
    if not (out.is_cuda and out.dtype in dtypes and tuple(out.shape) == shape and out.stride(-1) == 1
            and (not row_stride or out.stride(-2) >= row_stride)):
        kinds = " / ".join(str(d).replace("torch.", "") for d in dtypes)
        raise _lib.SwmhdError(f"{what}: out must be a {kinds} CUDA tensor of shape {shape} with unit stride in {axis_word}")
    return out


def cached_workspace(model, attr, need, dev):
    """The device workspace cached on the model as `attr`: grown to `need` doubles, the largest asked for so far."""
    ws = getattr(model, attr, None)
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = torch.empty((need,), dtype=torch.float64, device=dev)
        setattr(model, attr, ws)
    return ws


class DeviceTimeSeries:
    """A writer for run(): `capacity` samples of `names` in one device tensor, plus the host lists `times` and `iterations`.  The
    tensor is allocated when the first sample is written.  `write` only enqueues; `numpy` and `save` are the calls that synchronise.
    A subclass states _data (the name of the public tensor attribute, which it binds to `tensor`), _unit (what a slot holds, for the
    capacity message), dtype, _check_names(), _sample_shape(), _enqueue(out) and save(path)."""
    _data, _unit, dtype = "samples", "samples", torch.float64

    def __init__(self, model, names, schedule, capacity):
        self.model, self.names, self.schedule = model, tuple(names), schedule
        self._check_names()
        if capacity is None or int(capacity) < 1:
            raise _lib.SwmhdError(f"{type(self).__name__}: capacity ({self._unit}) must be given: the {self._data} stay on the device")
        self.capacity = int(capacity)
        self.times, self.iterations = [], []
        self._tensor = None

    def __len__(self):
        return len(self.times)

    @property
    def tensor(self):
        """The device tensor of all `capacity` slots; the first len(self) hold samples."""
        if self._tensor is None:
            self._tensor = torch.empty((self.capacity,) + self._sample_shape(), dtype=self.dtype, device=state_device(self.model))
        return self._tensor

    def write(self, time=None):
        """Enqueue one sample of the model's current state into the next slot."""
        k = len(self.times)
        if k >= self.capacity:
            raise _lib.SwmhdError(f"{type(self).__name__}: all {self.capacity} slots are written")
        self._enqueue(self.tensor[k])
        self.times.append(self.model.clock_time if time is None else time)
        self.iterations.append(self.model.iteration)

    def numpy(self):
        """The samples written so far as a host array (synchronises)."""
        return self.tensor[:len(self.times)].cpu().numpy()

    def _savez(self, path, **more):
        """One .npz: the samples under the public attribute's name, names, times, iterations and `more` (synchronises)."""
        import numpy as np
        np.savez(path, **{self._data: self.numpy()}, names=np.array(self.names), times=np.array(self.times, dtype=np.float64),
                 iterations=np.array(self.iterations, dtype=np.int64), **more)
