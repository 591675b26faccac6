"""Drop-ins for the initialisation pass that ``Trainer.init`` runs before the first step (LoG/utils/trainer.py:170-179): per
training view, over ALL points of the model,

* ``init_radius3d(self, batch, renderer)`` = ``Gaussian.init_radius3d`` (LoG/model/level_of_gaussian.py:55-63) ->
  ``(valid_flag bool[P], radius3d f32[P])``;
* ``log_init(self, renderer, batch, iteration)`` = ``LoG.init`` (:328-332): ``counter.radius3d_min`` updated in place,
  ``num_views += 1``, nothing read back;
* ``at_init_final(self)`` = ``LoG.at_init_final`` (:334-341): launches what is still pending, then the reference's own
  method, unchanged (its three ``.item()`` prints and its ``torch.maximum`` run once per training).

The reference activates every scale and rotation, calls ``compute_radius`` and then reads and writes through four boolean
masks, each a ``nonzero`` with a host synchronisation: some fifteen launches per view.  Here a view is one launch of
``lograst_init_radius3d`` on the RAW parameters (48 bytes read, at most 4 written per point), and because nothing a point
contributes but its radius depends on the camera, one launch takes many cameras: ``install(views_per_launch=K)`` keeps the
cameras of K calls of ``LoG.init`` in a table on the device and launches once for all of them.  The minimum does not depend
on the order of the views, so the result has the same bits for every K -- but with K > 1 ``counter.radius3d_min`` is
current only after ``flush(model)`` (``at_init_final`` does it).  The model's ``xyz``, ``scaling`` and ``rotation`` must
not change while views are pending: their ``_version`` and ``data_ptr`` are noted at the first pending view and compared
at every later one and at the flush.

``update_radius3d_min(xyz, scaling, rotation, cameras, radius3d_min)`` is the same launch without a LoG model.

The camera conventions stay the reference's: ``renderer.prepare_camera(batch, 0, renderer.background)`` is called as the
reference calls it, and the rasterizer's ``raster_settings`` are read.  What the kernel does not cover goes to the
reference's own method, saved by ``install()`` (logged once, counted by reason): tensors that are not on the GPU or not
fp32, activations other than exp / normalize, a 3-D ``xyz`` (frames), 2^31 rows or more, ``scale_modifier != 1``, a
rasterizer without the fork's ``compute_radius`` (the reference's own error surfaces).

Install with ``log_amd.init_pass.install()`` or ``log_amd.install_all(device_init=True)``."""
import torch

from . import _lib
from . import rasterizer as _r
from ._dropin import DropIns, Fallback, check_activations, device_and_rows, tensor

_F32 = torch.float32
CAMERA_FLOATS = 36     # proj[16], view[16], fx, fy, tanfovx, tanfovy (include/lograst.h: lograst_init_radius3d)
_ACTIVATIONS = ({"scaling_activation": torch.exp, "rotation_activation": torch.nn.functional.normalize},
                "activations other than exp / normalize")
_PENDING = "_log_amd_init_pending"      # the attribute of the model that holds its pending views
_views_per_launch = 1


def _targets():
    from LoG.model.level_of_gaussian import Gaussian, LoG
    return {"init_radius3d": (Gaussian, "init_radius3d"), "log_init": (LoG, "init"), "at_init_final": (LoG, "at_init_final")}


dropins = DropIns("init_pass", _targets)
stats, reset_stats = dropins.stats, dropins.reset_stats


# ---- the camera table ------------------------------------------------------------------------------------------------

def _settings(camera):
    """A GaussianRasterizationSettings, or a rasterizer object that carries one."""
    return getattr(camera, "raster_settings", camera)


class CameraTable:
    """``capacity`` cameras as the kernel reads them, filled without a host synchronisation: the two matrices by device
    copies as the cameras arrive, the four scalars through one pinned row block when the table is handed to the launch."""

    def __init__(self, device, capacity):
        self.device, self.count = device, 0
        self.table = torch.empty((capacity, CAMERA_FLOATS), dtype=_F32, device=device)
        self.scalars = torch.empty((capacity, 4), dtype=_F32, pin_memory=True)

    def add(self, rs):
        if float(rs.scale_modifier) != 1.0:
            raise Fallback("scale_modifier != 1")
        row = self.table[self.count]
        for at, m in ((0, rs.projmatrix), (16, rs.viewmatrix)):
            if not torch.is_tensor(m) or m.device != self.device:
                raise Fallback("tensors are not on the GPU")
            if m.numel() != 16:
                raise ValueError(f"camera matrix of shape {tuple(m.shape)}")
            row[at:at + 16].copy_(m.detach().reshape(16))
        tanfovx, tanfovy = float(rs.tanfovx), float(rs.tanfovy)
        s = self.scalars[self.count]
        s[0], s[1] = rs.image_width / (2.0 * tanfovx), rs.image_height / (2.0 * tanfovy)     # level_of_gaussian.py:79-80
        s[2], s[3] = tanfovx, tanfovy
        self.count += 1

    def finish(self):
        """-> the [count, 36] table, complete in stream order."""
        n = self.count
        if n:
            self.table[:n, 32:].copy_(self.scalars[:n], non_blocking=True)
        return self.table[:n]


# ---- the launch ------------------------------------------------------------------------------------------------------

def _model_inputs(g):
    """-> (device, P, xyz, scaling, rotation) of a Gaussian model the kernel covers."""
    device, P = device_and_rows(g.xyz)
    if g.xyz.dim() != 2:
        raise Fallback("a 3-D xyz (frames)")
    check_activations(getattr(g, "activation", None), *_ACTIVATIONS)
    return (device, P, tensor(g.xyz, device, _F32, (P, 3), "xyz"), tensor(g.scaling, device, _F32, (P, 3), "scaling"),
            tensor(g.rotation, device, _F32, (P, 4), "rotation"))


def _in_place(t, device, P, what):
    """A [P] buffer the kernel updates in place: a contiguous copy will not do."""
    if torch.is_tensor(t) and not t.is_contiguous():
        raise Fallback(f"{what} that is not contiguous")
    return tensor(t, device, _F32, (P,), what)


def _launch(device, P, xyz, scaling, rotation, table, radius3d_min, valid=None, radius3d=None):
    L = _r.HipBackend.require(device)
    with torch.cuda.device(device):
        _lib.check(L.lograst_init_radius3d(P, _r._ptr(xyz), _r._ptr(scaling), _r._ptr(rotation), int(table.shape[0]),
                                           _r._ptr(table), _r._ptr(radius3d_min), _r._ptr(valid), _r._ptr(radius3d),
                                           _r._stream_ptr(device)))


def update_radius3d_min(xyz, scaling, rotation, cameras, radius3d_min):
    """``radius3d_min`` (fp32[P], in place) after ``LoG.init`` on every camera of ``cameras`` -- a sequence of
    GaussianRasterizationSettings or of rasterizer objects -- for the RAW parameters xyz [P, 3], scaling [P, 3] and
    rotation [P, 4] (exp / normalize are the kernel's): one launch, no host synchronisation.  -> radius3d_min."""
    device, P = xyz.device, int(xyz.shape[0])
    _r.HipBackend.require(device)
    if P >= 2 ** 31:
        raise ValueError("2^31 rows or more")
    try:
        x, s, q = (tensor(t, device, _F32, (P, w), name) for t, w, name in ((xyz, 3, "xyz"), (scaling, 3, "scaling"),
                                                                          (rotation, 4, "rotation")))
        rmin = _in_place(radius3d_min, device, P, "radius3d_min")
        table = CameraTable(device, max(len(cameras), 1))
        for camera in cameras:
            table.add(_settings(camera))
    except Fallback as why:      # no reference method stands behind this function
        raise ValueError(f"update_radius3d_min: {why}") from None
    with torch.no_grad():
        _launch(device, P, x, s, q, table.finish(), rmin)
    return radius3d_min


# ---- Gaussian.init_radius3d ------------------------------------------------------------------------------------------

def _rasterizer_settings(renderer, batch):
    camera, rasterizer, background = renderer.prepare_camera(batch, 0, renderer.background)
    if not hasattr(rasterizer, "compute_radius"):
        raise Fallback("a rasterizer without compute_radius")
    return rasterizer.raster_settings


@dropins.dropin
def init_radius3d(self, batch, renderer):
    """Gaussian.init_radius3d on the device: the one-view form of the kernel, both of its results."""
    device, P, xyz, scaling, rotation = _model_inputs(self)
    table = CameraTable(device, 1)
    table.add(_rasterizer_settings(renderer, batch))
    valid = torch.empty(P, dtype=torch.uint8, device=device)
    radius3d = torch.empty(P, dtype=_F32, device=device)
    _launch(device, P, xyz, scaling, rotation, table.finish(), None, valid, radius3d)
    return valid.view(torch.bool), radius3d


# ---- LoG.init --------------------------------------------------------------------------------------------------------

class _Pending:
    """The views of one model that wait for their launch, and what the model's parameters were when the first arrived."""

    def __init__(self, g, device, capacity):
        self.table = CameraTable(device, capacity)
        self.capacity = capacity
        self.seen = self.fingerprint(g)

    @staticmethod
    def fingerprint(g):
        return tuple((t._version, t.data_ptr()) for t in (g.xyz, g.scaling, g.rotation))

    def check(self, g):
        if self.fingerprint(g) != self.seen:
            raise _lib.LograstError(
                f"log_amd.init_pass: xyz, scaling or rotation changed while {self.table.count} view(s) of LoG.init were "
                f"pending (views_per_launch={self.capacity}); call log_amd.init_pass.flush(model) before changing the model")


def flush(model):
    """Launch the views of ``model`` that ``LoG.init`` has enqueued (``install(views_per_launch=K)``, K > 1); after it
    ``model.counter.radius3d_min`` is current.  Nothing to do when nothing is pending."""
    pending = getattr(model, _PENDING, None)
    if pending is None or pending.table.count == 0:
        return
    g = model.gaussian
    pending.check(g)
    setattr(model, _PENDING, None)
    with torch.no_grad():
        device, P, xyz, scaling, rotation = _model_inputs(g)
        rmin = _in_place(model.counter.radius3d_min, device, P, "radius3d_min")
        _launch(device, P, xyz, scaling, rotation, pending.table.finish(), rmin)


@dropins.dropin
def log_init(self, renderer, batch, iteration):
    """LoG.init on the device.  views_per_launch == 1: launched at once; K > 1: enqueued, launched with the K-th."""
    g = self.gaussian
    device, P, xyz, scaling, rotation = _model_inputs(g)
    rmin = _in_place(self.counter.radius3d_min, device, P, "radius3d_min")
    rs = _rasterizer_settings(renderer, batch)
    pending = getattr(self, _PENDING, None)
    if pending is not None:
        pending.check(g)
    else:
        pending = _Pending(g, device, _views_per_launch)
    pending.table.add(rs)        # a Fallback here leaves the table as it was
    if pending.table.count >= pending.capacity:
        setattr(self, _PENDING, None)
        _launch(device, P, xyz, scaling, rotation, pending.table.finish(), rmin)
    else:
        setattr(self, _PENDING, pending)
    self.num_views += 1


@dropins.register
def at_init_final(self):
    """LoG.at_init_final: the pending views, then the reference's own method."""
    dropins.count("calls", "at_init_final")
    flush(self)
    return dropins.original("at_init_final")(self)


# ---- installation ----------------------------------------------------------------------------------------------------

def set_views_per_launch(k):
    """How many calls of ``LoG.init`` share one launch from now on (views already pending keep the table they have)."""
    global _views_per_launch
    k = int(k)
    if k < 1:
        raise ValueError("views_per_launch must be at least 1")
    _views_per_launch = k


def install(views_per_launch=1):
    """Patch the reference classes in place (needs LoG importable); the original methods are kept for the fall-backs.
    views_per_launch = K > 1: ``LoG.init`` launches once per K views, and ``counter.radius3d_min`` is current only after
    ``flush(model)`` or ``at_init_final``."""
    set_views_per_launch(views_per_launch)
    return dropins.install()["log_init"][0]


def uninstall():
    """Put the reference's methods back; ``views_per_launch`` returns to 1."""
    set_views_per_launch(1)
    dropins.uninstall()
