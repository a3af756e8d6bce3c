"""What the bindings of the companion interfaces share (streams.py ``sfm_*``, map_window.py ``sfw_*``, view.py ``sfv_*``,
score.py ``sfs_*``, keyframes.py ``sfk_*``, regions.py ``sfr_*``, align.py ``sfa_*``, join.py ``sfj_*``, tracks.py ``sft_*``, bodies.py ``sfb_*``, body_maps.py ``sfp_*``, deform.py ``sfd_*``, closure.py ``sfc_*``, carve.py ``sfe_*``, register.py ``sfg_*``). Their symbols are not part of the ABI of include/sf.h -- the CPU oracle does not have them -- so each
has a table of its own, bound to the HIP library of an `Api` (the very ``ctypes.CDLL`` object: one copy of the library,
one `sf_last_error`). Nothing here computes anything.
"""
import ctypes as C

from ._capi import SfError


class _Binding:
    def __init__(self, api, prefix, subject, signatures, version, sizes):
        if api.prefix != "sf_":
            raise SfError("%s implemented by the HIP library only (this binding has the prefix %r)" % (subject, api.prefix))
        self.api, self.prefix = api, prefix
        for name, (res, args) in signatures.items():
            fn = getattr(api.lib, name)  # AttributeError if the library lacks the symbol
            fn.restype = res
            fn.argtypes = args
            setattr(self, name[4:], fn)
        if self.version() != version:
            raise SfError("%s: %sversion %d, this binding restates %d" % (api.lib_path, prefix, self.version(), version))
        for fn, struct, size in sizes:
            if getattr(self, fn)() != size:
                raise SfError("%s: %s has %d bytes, this binding's %d" % (api.lib_path, struct, getattr(self, fn)(), size))

    def check(self, code, what):
        if code != 0:
            msg = self.api.last_error()
            raise SfError("%s%s failed with %d: %s" % (self.prefix, what, code, msg.decode() if msg else ""))


def binder(prefix, subject, signatures, version, sizes=()):
    """(_bind, _product) of a companion module. _bind(api): the functions of `signatures` on api's library as attributes
    without their four-character prefix, `.api` and `.check(code, what)`, made once per library path; refused for a library
    that is not the HIP one, whose ``<prefix>version()`` is not `version`, or where a (size function, struct name, bytes) of
    `sizes` disagrees. _product(): the same for the product library."""
    bound = {}

    def _bind(api):
        b = bound.get(api.lib_path)
        if b is None:
            b = bound[api.lib_path] = _Binding(api, prefix, subject, signatures, version, sizes)
        return b

    def _product():
        from . import load

        return _bind(load())

    return _bind, _product


class HandleChild:
    """base of the wrappers over what a binding creates from a solver's handle (sfk_db, sft_tracker, sfd_graph, sfc_builder, sfe_carver, sfg_registrar):
    `.solver`, `.api`, the binding `.b`, the pointer under the attribute `_ptr` names, `close()` -- the destroy function
    `_destroy` names, once, then a null pointer -- and a `__del__` that swallows"""

    _ptr = _destroy = None

    def __init__(self, solver, binding):
        self.solver, self.api, self.b = solver, solver.api, binding
        setattr(self, self._ptr, C.c_void_p())

    def close(self):
        if getattr(self, self._ptr, None):
            getattr(self.b, self._destroy)(getattr(self, self._ptr))
            setattr(self, self._ptr, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def one_solver(maps):
    if maps and any(m.solver is not maps[0].solver for m in maps):
        raise SfError("the maps of one call belong to one solver")


def map_array(maps):
    """the sf_map pointers of a batch"""
    return (C.c_void_p * max(len(maps), 1))(*[m.m.value for m in maps])


def ptr_array(items, n):
    """n void pointers from numpy arrays (their data) or integer addresses, None for a null entry; None for no list at all"""
    if items is None:
        return None
    return (C.c_void_p * n)(*[None if x is None else (x.ctypes.data if hasattr(x, "ctypes") else int(x)) for x in items])
