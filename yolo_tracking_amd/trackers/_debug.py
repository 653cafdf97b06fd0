"""Test-only read-back of the OC-SORT family's stage-1 matrices (yta_<t>_debug_costs).

The asso / embedding / cost matrices of a frame's first association round are overwritten by the
frame's later rounds, so an engine keeps a copy only while the switch is on: `debug_costs_enable()`
once, then `debug_costs(stream)` after each `update()`.  `update_tensors()` refuses while it is on.
"""
import numpy as np

from .. import _lib


class DebugCosts:
    # the C call's arrays after `ids`, in order: (name, kind), kind "m" an n_high x n_trk matrix,
    # "r" one value per row, "c" one per column
    _debug_fields = ()

    def debug_costs_enable(self, on=True):
        fn = getattr(self.lib, f"yta_{self._abi}_debug_costs_enable")
        _lib.check(fn(self._h, int(bool(on))))

    def debug_costs(self, stream=0):
        """The last update()'s stage-1 matrices of one stream as NumPy arrays: n_high, n_trk, rows
        (the input-row index of each matrix row), ids and boxes (the track id and the predicted
        box x1, y1, x2, y2 of each matrix column) and the engine's matrices (see the engine's class
        docstring)."""
        fn = getattr(self.lib, f"yta_{self._abi}_debug_costs")
        dims = np.zeros(4, dtype=np.int32)
        null = [None] * (3 + len(self._debug_fields))
        _lib.check(fn(self._h, int(stream), _lib.ptr(dims), *null))
        m, n = int(dims[0]), int(dims[1])
        rows = np.zeros(m, dtype=np.int32)
        ids = np.zeros(n, dtype=np.int64)
        boxes = np.zeros((n, 4), dtype=np.float64)
        shape = {"m": (m, n), "r": (m,), "c": (n,)}
        arrs = [np.zeros(shape[kind], dtype=np.float64) for _, kind in self._debug_fields]
        _lib.check(fn(self._h, int(stream), _lib.ptr(dims), *[_lib.ptr(a) if a.size else None
                                                             for a in [rows, ids, boxes] + arrs]))
        assert (int(dims[0]), int(dims[1])) == (m, n)
        out = dict(n_high=m, n_trk=n, rows=rows, ids=ids, boxes=boxes, dims=dims.copy())
        out.update({name: a for (name, _), a in zip(self._debug_fields, arrs)})
        return out


__all__ = ["DebugCosts"]
