"""LoG's depth pass inside the colour pass: one rasterizer call per depth-supervised view instead of two.

With ``render_depth: True`` the reference's ``NaiveRendererAndLoss.render`` (LoG/render/renderer.py:117-205) calls the
rasterizer twice on the same Gaussians: at :153 with the RGB colours, at :190 with ``colors_precomp = [view z, world z, 1]``.
The rasterizer here composites a second colour triple in the same walk (``GaussianRasterizer.forward(aux_colors=)``), so
the wrapped ``render`` hands the reference's own ``render`` a proxy around the rasterizer object:

* the proxy's first call builds ``[view z, world z, 1]`` from its ``means3D`` and the camera's ``world_view_transform`` with
  the torch operations of renderer.py:167-169,187-189 (``cat``, ``@``, select, ``ones_like``, ``stack``: the reference's bits,
  and autograd ties world z to ``xyz``), passes it as ``aux_colors`` and keeps the returned ``aux_image``;
* the second call -- the same ``means3D`` / ``opacities`` / ``scales`` / ``rotations`` objects, a ``colors_precomp`` of
  shape [N, 3], no ``shs`` -- launches nothing: it returns the kept ``aux_image`` in place 0 with the first call's ``radii``
  and maps.

Anything else goes to the real rasterizer and is counted by reason (``stats()``).  ``render`` itself is not restated: every
key of its output is what the reference leaves.  The reference still builds its own ``colors_depth`` (five small launches);
``set_verify(True)`` compares it with what the first call composited (synchronises: tests and debugging).

* ``install()`` / ``uninstall()``: ``NaiveRendererAndLoss.render`` (``MaskForeground`` inherits it);
  ``log_amd.install_all(fused_depth_pass=True)`` calls it.
* ``wrap_render(fn)``: the same wrapper around any ``render``-like function that takes ``camera`` and ``rasterizer``."""
import functools
import inspect

import torch

from . import _lib
from . import rasterizer as _r
from ._dropin import DropIns


def _targets():
    import LoG.render.renderer as rr
    return {"render": (rr.NaiveRendererAndLoss, "render")}


_dropins = DropIns("depth_pass", _targets)
_verify = False
_GEOMETRY = ("means3D", "opacities", "scales", "rotations")


def set_verify(enabled):
    """True: the second call additionally checks ``torch.equal(colors_precomp, aux_colors)`` and raises LograstError on a
    mismatch (one host synchronisation per view).  Returns the previous setting."""
    global _verify
    prev, _verify = _verify, bool(enabled)
    return prev


def stats():
    """{'calls': wrapped render calls, 'fused': views whose depth call launched nothing, 'fallback': {reason: n}} since the
    last reset; a fallback is a rasterizer call (or a whole render) that went to the real rasterizer."""
    s = _dropins.stats()
    return dict(calls=s["calls"].get("render", 0), fused=s["calls"].get("fused", 0),
                fallback={why: n for (_, why), n in s["fallbacks"].items()})


def reset_stats():
    _dropins.reset_stats()


def _fallback(why):
    _dropins.count("fallbacks", ("render", why))


class _RasterizerProxy:
    """Stands where the rasterizer object stands for ONE call of ``render``; everything but ``__call__`` is the real
    object's (raster_settings, compute_radius, ...)."""

    def __init__(self, rasterizer, camera):
        self.__dict__.update(_rast=rasterizer, _camera=camera, _calls=0, _kept=None)

    def __getattr__(self, name):
        return getattr(self._rast, name)

    def __setattr__(self, name, value):
        setattr(self._rast, name, value)

    def _covered(self, args, kw):
        """-> the reason why this first call is not fused, or None."""
        if args:
            return "positional arguments"
        if kw.get("cov3D_precomp") is not None or kw.get("scales") is None or kw.get("rotations") is None:
            return "cov3D_precomp"
        if not hasattr(_r._backend, "forward_aux"):
            return "the backend has no forward_aux"
        m = kw.get("means3D")
        on_gpu = not isinstance(_r._backend, _r.HipBackend)     # (a test double takes the tensors it takes)
        if not all(torch.is_tensor(kw.get(k)) and (on_gpu or kw[k].device.type == "cuda") and kw[k].device == m.device
                   for k in _GEOMETRY):
            return "tensors are not on the GPU"
        if kw.get("use_filter", True) is not True:
            return "use_filter differs between the two calls"     # (renderer.py:151-152 sets it on the first call only)
        if "aux_colors" in kw:
            return "the caller passes aux_colors itself"
        if _r._tile_rows.get() != (0, 0):
            return "tile_rows band"
        if _r._grad_sink is not None:
            return "accumulate_grads_into"
        abs_own = getattr(self._rast, "abs_grad", None)
        if _r._abs_grad_on() if abs_own is None else abs_own:
            return "abs_grad"     # (no abs form of the aux backward: both calls are real, their abs sums add on the shared means2D)
        wvt = self._camera.get("world_view_transform") if hasattr(self._camera, "get") else None
        if not torch.is_tensor(wvt) or wvt.device != m.device:
            return "the camera's world_view_transform is not on the tensors' device"
        return None

    def __call__(self, *args, **kw):
        self.__dict__["_calls"] += 1
        if self._calls == 1:
            why = self._covered(args, kw)
            if why is not None:
                _fallback(why)
                return self._rast(*args, **kw)
            xyz = kw["means3D"]
            xyz1 = torch.cat([xyz.detach(), torch.ones_like(xyz[:, :1])], dim=1)               # renderer.py:167-169
            point_depth = (xyz1 @ self._camera["world_view_transform"])[:, 2]
            aux = torch.stack([point_depth, xyz[:, 2], torch.ones_like(point_depth)], dim=-1)  # renderer.py:187-189
            ret = self._rast(aux_colors=aux, **kw)
            self.__dict__["_kept"] = dict(aux=aux, aux_image=ret[-1], rest=tuple(ret[1:-1]),
                                          geometry=tuple(kw.get(k) for k in _GEOMETRY))
            return tuple(ret[:-1])
        kept, self.__dict__["_kept"] = self._kept, None
        if self._calls == 2 and kept is not None:
            c = kw.get("colors_precomp")
            same = (not args and kw.get("shs") is None and kw.get("cov3D_precomp") is None and "use_filter" not in kw
                    and torch.is_tensor(c) and tuple(c.shape) == tuple(kept["aux"].shape)
                    and all(kw.get(k) is g for k, g in zip(_GEOMETRY, kept["geometry"])))
            if same:
                if _verify and not torch.equal(c.detach(), kept["aux"].detach()):
                    raise _lib.LograstError("log_amd.depth_pass: the depth call's colors_precomp is not the [view z, world z, 1] "
                                            "that the first call composited")
                _dropins.count("calls", "fused")
                return (kept["aux_image"],) + kept["rest"]
            _fallback("the second call has other tensors")
        elif self._calls >= 3:
            _fallback("more than two calls")
        else:
            _fallback("the second call follows an unfused first call")
        return self._rast(*args, **kw)


def wrap_render(original):
    """-> a function with ``original``'s signature (it must take ``self``, ``camera`` and ``rasterizer``) that, when
    ``self.render_depth`` is true, calls ``original`` with a proxy in place of the rasterizer."""
    sig = inspect.signature(original)
    if "camera" not in sig.parameters or "rasterizer" not in sig.parameters:
        raise TypeError("wrap_render: the function must take `camera` and `rasterizer`")

    @functools.wraps(original)
    def render(self, *args, **kwargs):
        if not getattr(self, "render_depth", False):
            return original(self, *args, **kwargs)
        _dropins.count("calls", "render")
        if getattr(self, "use_origin_render", False):
            _fallback("use_origin_render")
            return original(self, *args, **kwargs)
        bound = sig.bind(self, *args, **kwargs)
        bound.arguments["rasterizer"] = _RasterizerProxy(bound.arguments["rasterizer"], bound.arguments["camera"])
        return original(*bound.args, **bound.kwargs)
    render._lograst_original = original
    return render


def install():
    """Patch the reference in place (needs LoG.render.renderer importable): NaiveRendererAndLoss.render."""
    targets = _targets()
    cls, attr = targets["render"]
    if not hasattr(getattr(cls, attr), "_lograst_original"):
        _dropins.register(wrap_render(_dropins.original("render")), name="render")
        _dropins.install()
    return cls


def uninstall():
    """Put back what install() replaced."""
    import sys
    if sys.modules.get("LoG.render.renderer") is not None:
        _dropins.uninstall()
