"""Id selectors for the subset search of the flat dense indexes, `IVFFlatIndex`, `PQIndex` and `IVFPQIndex`: `index.search(x, k,
params=SearchParameters(sel=...))`, the names and meanings of Faiss's `IDSelector` family (not in the reference, which only ever
searches whole stores).

A selector holds EXTERNAL ids (row + the index's `id_offset`).  `sel.rows(ntotal, id_offset, device)` turns it into what the
kernels read: the int64 rows inside [0, ntotal), strictly ascending, no row twice (`ops.dense_search(rows=...)`).  Ids outside
the index are ignored and duplicates collapse — a Faiss selector's `is_member` simply never matches them — so the list is
valid by construction and the indexes pass it on with `check_rows=False`.  The list is cached on the selector per
(ntotal, id_offset, device): a selector reused across batches is built once, and an index that has grown builds it again.
`IVFFlatIndex` keeps its rows list-major, not in corpus order: it takes the selector's `_mask` and builds its own pair
(positions, offsets per cell) from it, cached on the selector too (`IVFFlatIndex._selection`).
`PQIndex` and `IVFPQIndex` take the same selectors by compaction: the selected codes and their permuted image are gathered once
into a selection that the unchanged ADC search scans (`PQIndex._selection`, `IVFPQIndex._selection`, `ops.adc_select_rows`), cached
on the selector as well, one entry (`_adc`).
Everything here is torch on whatever device is asked for, CPU included; nothing loads the library.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch


def _ids_tensor(ids) -> torch.Tensor:
    t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ids))
    if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError("selector: a 1-d array of integer ids")
    return t.to(torch.int64)


class IDSelector:
    """Base of the selectors: `rows` with its one-entry cache around the subclass's `_build`."""

    def __init__(self):
        self._key = None
        self._rows = None
        self._ivf_key = None          # IVFFlatIndex._selection's one-entry cache: the store's generation number (unique over
                                      # all indexes, so it names the index too) ...
        self._ivf = None              # ... and the (rows, sel_off, sizes_desc) built for it
        self._adc_key = None          # PQIndex._selection's / IVFPQIndex._selection's one-entry cache: the generation number of the
                                      # codes (unique over those indexes) with what else the selection depends on ...
        self._adc = None              # ... and the selection: compact codes, their image, the row list (~2 ns M bytes)

    def rows(self, ntotal: int, id_offset: int = 0, device=None) -> torch.Tensor:
        """int64 [ns]: the rows r in [0, ntotal), ascending and unique, whose id r + id_offset the selector holds."""
        device = torch.device("cpu" if device is None else device)
        key = (int(ntotal), int(id_offset), device)
        if self._key != key:
            self._rows = self._build(int(ntotal), int(id_offset), device).contiguous()
            self._key = key
        return self._rows

    def _mask(self, ntotal: int, id_offset: int, device) -> torch.Tensor:
        """bool [ntotal]: row r is selected."""
        m = torch.zeros((ntotal,), dtype=torch.bool, device=device)
        m[self.rows(ntotal, id_offset, device)] = True
        return m

    def _build(self, ntotal: int, id_offset: int, device) -> torch.Tensor:
        raise NotImplementedError


class IDSelectorRange(IDSelector):
    """The ids in [imin, imax) (half-open, as Faiss's).  The flat indexes search the matching slice of the store as a view and
    take no row list for it (`span`)."""

    def __init__(self, imin: int, imax: int):
        super().__init__()
        self.imin, self.imax = int(imin), int(imax)

    def span(self, ntotal: int, id_offset: int = 0):
        """(lo, hi): the selected rows are exactly lo .. hi - 1, lo <= hi, inside [0, ntotal]."""
        lo = min(max(self.imin - int(id_offset), 0), int(ntotal))
        hi = min(max(self.imax - int(id_offset), lo), int(ntotal))
        return lo, hi

    def _build(self, ntotal, id_offset, device):
        lo, hi = self.span(ntotal, id_offset)
        return torch.arange(lo, hi, dtype=torch.int64, device=device)


class IDSelectorBatch(IDSelector):
    """The ids of an array (numpy or tensor, any integer type); ids the index does not hold are ignored, repeats collapse."""

    def __init__(self, ids):
        super().__init__()
        self.ids = _ids_tensor(ids)

    def _build(self, ntotal, id_offset, device):
        r = self.ids.to(device) - id_offset
        return torch.unique(r[(r >= 0) & (r < ntotal)])            # sorted ascending


IDSelectorArray = IDSelectorBatch       # Faiss's two names for "these ids"; here both are the sorted, de-duplicated list


class IDSelectorBitmap(IDSelector):
    """Faiss's bitmap: id i is selected iff bit (i & 7) of byte (i >> 3) of `bits` (uint8) is set; ids past the bitmap are not."""

    def __init__(self, bits):
        super().__init__()
        t = bits if isinstance(bits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(bits))
        if t.dim() != 1 or t.dtype != torch.uint8:
            raise ValueError("IDSelectorBitmap: a 1-d uint8 array")
        self.bits = t

    def _build(self, ntotal, id_offset, device):
        ids = torch.arange(ntotal, dtype=torch.int64, device=device) + id_offset
        inside = (ids >= 0) & (ids < 8 * self.bits.numel())
        ids = ids[inside]
        byte = self.bits.to(device)[ids >> 3].to(torch.int64)
        rows = ids[((byte >> (ids & 7)) & 1) != 0] - id_offset
        return rows


class IDSelectorNot(IDSelector):
    """Every id of the index that `sel` does not hold."""

    def __init__(self, sel: IDSelector):
        super().__init__()
        if not isinstance(sel, IDSelector):
            raise ValueError("IDSelectorNot: an IDSelector")
        self.sel = sel

    def _build(self, ntotal, id_offset, device):
        return torch.nonzero(~self.sel._mask(ntotal, id_offset, device)).flatten()


class SearchParameters:
    """`params` of the flat indexes' `search`: `sel`, an IDSelector or None (the whole store, today's path bit for bit)."""

    def __init__(self, sel: Optional[IDSelector] = None):
        if sel is not None and not isinstance(sel, IDSelector):
            raise ValueError("SearchParameters: sel must be an IDSelector or None")
        self.sel = sel


class SearchParametersIVF(SearchParameters):
    """Faiss's `SearchParametersIVF`: `sel` as above, and `nprobe`, the cells probed by this call (None: the index's
    attribute).  `IVFFlatIndex.search` takes either class; its explicit `nprobe=` argument wins over this one."""

    def __init__(self, sel: Optional[IDSelector] = None, nprobe: Optional[int] = None):
        super().__init__(sel)
        if nprobe is not None and (isinstance(nprobe, bool) or int(nprobe) != nprobe or int(nprobe) < 1):
            raise ValueError("SearchParametersIVF: nprobe must be an integer >= 1 or None")
        self.nprobe = None if nprobe is None else int(nprobe)
