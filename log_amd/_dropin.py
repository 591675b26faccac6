"""What every module of drop-ins with a fall-back shares (densify, prepare, decide, evaluate): the ``Fallback`` exception, the
registry that saves the reference's methods, installs ours, counts and logs, the checks of what the kernels cover, and the
launch whose result the host reads back.  A module keeps what is its own: what it checks, launches and prints.

    dropins = DropIns("prepare", lambda: {"clamp_scale": (LoG, "clamp_scale")})      # the classes, imported lazily

    @dropins.dropin
    def clamp_scale(self, index):          # the device body: raises Fallback(reason) for what the kernels do not cover
        ...

The other modules keep their own conventions: lod, counter, sparse_optimizer and get_all overwrite methods and have no
fall-back; loss and depth_loss wrap theirs behind a predicate."""
import contextlib
import functools
import inspect
import logging

import torch

from . import _lib
from . import rasterizer as _r

TREE_DTYPES = {"node_index": torch.int32, "index_parent": torch.int32, "local_index": torch.int8, "depth": torch.int8}


class Fallback(Exception):
    """Raised inside a drop-in for a case the kernels do not cover; the reference's method then runs."""


class DropIns:
    """The drop-ins of one module.  ``targets()`` -> {name: (class, attribute)}: where each registered function goes."""

    def __init__(self, module, targets):
        self.module, self._targets = module, targets
        self._ours = {}                # name -> our function
        self._saved = {}               # name -> the reference's method, saved on first need
        self._static = set()           # the names whose target is a staticmethod
        self.logged = set()            # the (method, reason) pairs that have had their warning
        self._stats = {"calls": {}, "fallbacks": {}, "readbacks": {}}

    # ---- the public functions ----

    def register(self, fn=None, *, name=None):
        """Decorator: ``fn`` is what install() puts in place of the reference's method of that name (``name``: where the
        function's own name is another)."""
        if fn is None:
            return lambda f: self.register(f, name=name)
        self._ours[name or fn.__name__] = fn
        return fn

    def dropin(self, body):
        """Decorator: the device body becomes the registered drop-in -- counted, run without grad, and handed over to the
        reference's method with the caller's own arguments when the body raises Fallback."""
        @functools.wraps(body)
        def public(*args, **kwargs):
            return self.run(body.__name__, body, *args, **kwargs)
        return self.register(public)

    def run(self, name, body, *args, **kwargs):
        self.count("calls", name)
        try:
            with torch.no_grad():
                return body(*args, **kwargs)
        except Fallback as why:
            return self.fall_back(name, why, *args, **kwargs)

    def fall_back(self, name, why, *args, **kwargs):
        """Counts and logs (once per method and reason) the fall-back, then -> the reference's method's result."""
        why = str(why)
        self.count("fallbacks", (name, why))
        if (name, why) not in self.logged:
            self.logged.add((name, why))
            logging.getLogger("log_amd").warning("log_amd.%s.%s: %s -- the reference's method runs instead (logged once)",
                                                 self.module, name, why)
        return self.original(name)(*args, **kwargs)

    # ---- statistics ----

    def count(self, kind, key, n=1):
        self._stats[kind][key] = self._stats[kind].get(key, 0) + n

    def stats(self):
        """{'calls': {method: n}, 'fallbacks': {(method, reason): n}, 'readbacks': {method: n}} since the last reset:
        read-backs are the library's ``*_read`` calls (one stream synchronisation each) made on behalf of a method."""
        return {k: dict(v) for k, v in self._stats.items()}

    def reset_stats(self):
        for v in self._stats.values():
            v.clear()

    # ---- installation ----

    def original(self, name):
        if name not in self._saved:
            cls, attr = self._targets()[name]
            fn = getattr(cls, attr)
            if isinstance(inspect.getattr_static(cls, attr, None), staticmethod):
                self._static.add(name)         # a plain setattr would make an instance method of it: see _put
            if fn in self._ours.values():
                raise _lib.LograstError(f"log_amd.{self.module}: the reference's {attr} was replaced before install() "
                                        f"could save it")
            self._saved[name] = fn
        return self._saved[name]

    @contextlib.contextmanager
    def substituted(self, **originals):
        """Inside the block the given functions stand where the saved originals do (a test's stand-in reference)."""
        saved = dict(self._saved)
        self._saved.update(originals)
        try:
            yield
        finally:
            self._saved.clear()
            self._saved.update(saved)

    def _put(self, target, name, fn):
        setattr(*target, staticmethod(fn) if name in self._static else fn)

    def install(self):
        """Saves the reference's methods, then puts ours in their place -> targets().  A registered name that targets()
        leaves out (its module cannot be imported) is skipped."""
        targets = self._targets()
        names = [name for name in self._ours if name in targets]
        for name in names:
            self.original(name)
        for name in names:
            self._put(targets[name], name, self._ours[name])
        return targets

    def uninstall(self):
        """Put the reference's methods back."""
        targets = self._targets()
        for name, fn in self._saved.items():
            if name in targets:
                self._put(targets[name], name, fn)

    # ---- a launch whose result the host needs ----

    def launch_and_read(self, who, device, nbytes, launch, read):
        """``launch(scratch, nbytes, stream)`` then ``read(scratch, stream)`` on the current stream of ``device``, over
        ``nbytes`` of fresh scratch: one read-back counted for ``who`` -> the scratch."""
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            stream = _r._stream_ptr(device)
            _lib.check(launch(_r._ptr(scratch), nbytes, stream))
            _lib.check(read(_r._ptr(scratch), stream))
        self.count("readbacks", who)
        return scratch


# ---- what the kernels cover: one definition per check ----------------------------------------------------------------

def device_and_rows(t):
    """-> (device, rows) of a tensor the kernels can index: on the GPU, fewer than 2^31 rows."""
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise Fallback("tensors are not on the GPU")
    p = int(t.shape[0])
    if p >= 2 ** 31:
        raise Fallback("2^31 rows or more")
    return t.device, p


def tensor(t, device, dtype, shape, what):
    """A buffer as the kernels read it: on ``device``, of that dtype and shape, detached and contiguous."""
    if not torch.is_tensor(t) or t.device != device:
        raise Fallback("tensors are not on the GPU")
    if t.dtype != dtype or tuple(t.shape) != shape:
        raise Fallback(f"{what}: {t.dtype}{tuple(t.shape)} where {dtype}{shape} is needed")
    return t.detach().contiguous()


def flag_u8(flag, device, p):
    """A bool or integer flag per row as the uint8[p] the kernels read."""
    if not torch.is_tensor(flag) or flag.device != device:
        raise Fallback("flags are not on the model's device")
    if flag.dim() != 1 or int(flag.shape[0]) != p:
        raise ValueError(f"flag of shape {tuple(flag.shape)} for {p} rows")
    f = flag.detach().contiguous()
    return f.view(torch.uint8) if f.dtype == torch.bool else (f != 0).view(torch.uint8)


def tree_buffers(tree, device, p, names=tuple(TREE_DTYPES)):
    """-> {name: the tree's per-row buffer, contiguous}, each of its TREE_DTYPES dtype, [p], on ``device``."""
    arrays = {}
    for name in names:
        t, dt = getattr(tree, name), TREE_DTYPES[name]
        if t.device != device:
            raise Fallback("tree buffers are not on the model's device")
        if t.dtype != dt or t.dim() != 1 or int(t.shape[0]) != p:
            raise ValueError(f"tree buffer {name}: expected {dt}[{p}], got {t.dtype}{tuple(t.shape)}")
        arrays[name] = t.contiguous()
    return arrays


def check_activations(act, want, words):
    """want: {attribute of the model's activation object: the function the kernels compute}; words: the reason."""
    if act is None or any(getattr(act, name, None) is not fn for name, fn in want.items()):
        raise Fallback(words)
