"""Python handle on one device context of the C-ABI (include/doorman_hip.h).

This is a thin binding used by tests and bench.py; the store, the planner and
the kernels live in libdoorman_hip.so.  Method names follow the reference's
LeaseStore / Algorithm surface (go/server/doorman/store.go:68-103,
algorithm.go:44) where one exists.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib
from .workloads import CFG_FIELDS

_BIN_NAMES = ("small_tiles", "sub16x4", "sub32x4", "wave64x4", "block128x4", "block128x8", "block256x8",
              "block2k4k", "sub8x2", "sub16x2", "large_resources", "large_chunks", "leases", "bin_shapes",
              "redo_resident_cap", "spec_fits", "aux_own_queues", "stream_parts", "queue_perm", "wb_inplace",
              "steady_parts", "fixed_parts", "sweep_parts", "kept_refreshes", "cycle_parts", "masked_parts")
# dm_plan_info's slots beyond the bins' table, in order
_PLAN_NAMES = _BIN_NAMES + ("fused_parts", "told_listed", "told_queued", "rounds_in_tick")


def _ptr(a):
    return None if a is None else a.ctypes.data


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _host_col(a, dts):
    """A host column for _fill_batch: contiguous, of dtype dts[0] or, where it has it already,
    of dts[1]."""
    dt = dts[1] if len(dts) > 1 and np.asarray(a).dtype == dts[1] else dts[0]
    a = np.ascontiguousarray(a, dtype=dt)
    return a.ctypes.data, len(a), a


def _device_col(t, dts):
    """A device column for _fill_batch (checked by _check_device_col before)."""
    return t.data_ptr() or None, len(t), t


def _check_device_col(name, t, dts, noun, device):
    """One column of a device snapshot or a device update (the noun), checked without a context
    or a library call: a CUDA tensor of torch (or any object with data_ptr(), dtype, device and
    a length) on `device`, of one of the dtypes dts, one contiguous dimension."""
    import torch
    want = torch.device("cuda", device)
    if not hasattr(t, "data_ptr") or not hasattr(t, "device"):
        raise ValueError(f"{name} must be a tensor on {want} (data_ptr(), dtype, device and a length)")
    dev = torch.device(t.device)
    if dev.type != "cuda":
        raise ValueError(f"{name} is on {dev}: a device {noun}'s columns live on {want}")
    if dev.index is not None and dev.index != device:
        raise ValueError(f"{name} is on {dev}, the engine on {want}")
    if str(t.dtype).replace("torch.", "") not in dts:
        raise ValueError(f"{name} must be {' or '.join(dts)}, not {t.dtype}")
    if getattr(t, "ndim", 1) != 1 or (hasattr(t, "is_contiguous") and not t.is_contiguous()):
        raise ValueError(f"{name} must be one contiguous column")


def _fill_batch(col, wants_mask, wants, release_rows, upsert, wants_first_row, now_ns):
    """The StoreBatch of apply() and apply_device().  col(column, dtypes) gives a column's
    (pointer, length, object to keep alive while the library reads it): _host_col or
    _device_col.  Returns the batch and the kept objects."""
    if upsert is not None and upsert[4] is None and now_ns is None:
        raise ValueError("arrivals without expiries need now_ns (their expiry is now_ns + lease length)")
    b, keep = _lib.StoreBatch(), []

    def put(a, *dts):
        p, n, k = col(a, dts)
        keep.append(k)
        return p, n, k

    if wants_mask is not None:
        b.wants_mask, b.wants_nwords, _ = put(wants_mask, "uint64", "int64")
        b.wants_first_row = int(wants_first_row)
        if wants is not None:
            b.wants, b.wants_n, _ = put(wants, "float64")
    if release_rows is not None:
        b.release_rows, b.release_n, _ = put(release_rows, "int64")
    if upsert is not None:
        rows, has, wv, sub, exp = upsert
        b.upsert_rows, b.upsert_n, _ = put(rows, "int64")
        if has is not None:
            b.upsert_has = put(has, "float64")[0]
        b.upsert_wants = put(wv, "float64")[0]
        p, _, k = put(sub, "int64", "int32")
        if str(k.dtype).replace("torch.", "") == "int32":
            b.upsert_subclients32 = p
        else:
            b.upsert_subclients = p
        if exp is not None:
            b.upsert_expiry_ns = put(exp, "int64")[0]
        b.upsert_now_ns = int(now_ns or 0)
    return b, keep


class Engine:
    """One GPU context owning a device-resident columnar lease store."""

    def __init__(self, device: int = 0, lib_path: str | None = None):
        self._L = _lib.lib(lib_path)
        self._ctx = ctypes.c_void_p()
        check(self._L.dm_create(device, ctypes.byref(self._ctx)), None, self._L)
        self.device = device
        self.n_resources = 0
        self.n_leases = 0
        self.seg_off = np.zeros(1, np.int64)
        self._pinned = []

    # -- lifetime --
    def host_empty(self, n: int, dtype=np.float64) -> np.ndarray:
        """A page-locked host array (dm_host_alloc), for update batches that should cross
        PCIe by DMA at full rate.  Valid until close()."""
        dtype = np.dtype(dtype)
        nbytes = max(int(n), 1) * dtype.itemsize
        ptr = ctypes.c_void_p()
        self._chk(self._L.dm_host_alloc(self._ctx, nbytes, ctypes.byref(ptr)))
        self._pinned.append(ptr.value)
        buf = (ctypes.c_byte * nbytes).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dtype, count=int(n))

    def close(self):
        if self._ctx:
            for ptr in getattr(self, "_pinned", []):
                self._L.dm_host_free(self._ctx, ctypes.c_void_p(ptr))
            self._pinned = []
            self._L.dm_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        return check(rc, self._ctx, self._L)

    @property
    def stream(self) -> int:
        return self._L.dm_get_stream(self._ctx) or 0

    def set_stream(self, stream_ptr: int | None):
        self._chk(self._L.dm_set_stream(self._ctx, stream_ptr))

    def sync(self):
        self._chk(self._L.dm_sync(self._ctx))

    def join(self):
        """dm_join: order deferred ticks before later work on the context stream."""
        self._chk(self._L.dm_join(self._ctx))

    def stream_wait(self, hip_stream: int):
        """dm_stream_wait: order hip_stream after the work enqueued so far on this engine."""
        self._chk(self._L.dm_stream_wait(self._ctx, ctypes.c_void_p(hip_stream)))

    # -- LeaseStore --
    def load(self, snap: dict):
        """NewLeaseStore + Assign of every row (store.go:114,153) and the resolved config."""
        self.load_store(snap)
        self.load_config(snap)

    def load_store(self, snap: dict):
        keep = {
            "seg_off": _c(snap["seg_off"], np.int64),
            "wants": _c(snap["wants"], np.float64),
            "has": _c(snap["has"], np.float64),
            "subclients": _c(snap["subclients"], np.int64),
            "expiry_ns": _c(snap["expiry_ns"], np.int64),
        }
        have = snap.get("agg_count") is not None
        if have:
            keep["agg_count"] = _c(snap["agg_count"], np.int64)
            keep["agg_sum_has"] = _c(snap["agg_sum_has"], np.float64)
            keep["agg_sum_wants"] = _c(snap["agg_sum_wants"], np.float64)
        s = _lib.Snapshot()
        s.n_resources = len(keep["seg_off"]) - 1
        s.n_leases = len(keep["wants"])
        for k in ("seg_off", "wants", "has", "subclients", "expiry_ns"):
            setattr(s, k, _ptr(keep[k]))
        if have:
            s.agg_count = _ptr(keep["agg_count"])
            s.agg_sum_has = _ptr(keep["agg_sum_has"])
            s.agg_sum_wants = _ptr(keep["agg_sum_wants"])
        self._chk(self._L.dm_store_load(self._ctx, ctypes.byref(s)))
        self.n_resources, self.n_leases = s.n_resources, s.n_leases
        self.seg_off = keep["seg_off"].copy()  # the table layout (host copy)

    def relayout(self, seg_off, compact: bool = False, want_row_map: bool = False):
        """dm_store_relayout: the same rows under a new seg_off, moved on the device (resources
        grow, shrink or are appended: len(seg_off) - 1 >= n_resources).  Default: each
        resource's rows keep their offsets, new tail rows are free; compact: its rows that are
        not released move to the front of its segment.  Returns the row map (new row of every
        old row, -1 for a dropped released row) when asked for, else None."""
        off = _c(seg_off, np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise ValueError("seg_off must hold n_resources + 1 offsets")
        row_map = np.empty(self.n_leases, np.int64) if want_row_map else None
        self._chk(self._L.dm_store_relayout(self._ctx, len(off) - 1, _ptr(off),
                                            _lib.DM_RELAYOUT_COMPACT if compact else 0, _ptr(row_map)))
        self.n_resources, self.n_leases = len(off) - 1, int(off[-1])
        self.seg_off = off.copy()
        return row_map

    def load_config(self, snap: dict):
        R = len(snap["kind"])
        keep = {
            "kind": _c(snap["kind"], np.int32),
            "capacity": _c(snap["capacity"], np.float64),
            "lease_length_s": _c(snap["lease_length_s"], np.int64),
            "refresh_interval_s": _c(snap["refresh_interval_s"], np.int64),
            "learning_end_ns": _c(snap["learning_end_ns"], np.int64),
            "parent_expiry_ns": _c(snap["parent_expiry_ns"], np.int64),
            "safe_capacity": _c(snap["safe_capacity"], np.float64),
        }
        cfg = _lib.ResourceCfg(*[_ptr(keep[k]) for k in CFG_FIELDS])
        self._chk(self._L.dm_config_load(self._ctx, R, ctypes.byref(cfg)))

    def upsert(self, rows, has, wants, subclients, expiry_ns):
        """Assign on existing rows (store.go:153-167)."""
        rows = _c(rows, np.int64)
        a = [_c(has, np.float64), _c(wants, np.float64), _c(subclients, np.int64), _c(expiry_ns, np.int64)]
        self._chk(self._L.dm_store_upsert(self._ctx, len(rows), _ptr(rows), *[_ptr(x) for x in a]))

    def update_wants(self, rows, wants):
        """Refresh that only changes wants (store.go:153-167, narrow form)."""
        rows, wants = _c(rows, np.int64), _c(wants, np.float64)
        self._chk(self._L.dm_store_update_wants(self._ctx, len(rows), _ptr(rows), _ptr(wants)))

    def update_wants_mask(self, mask, wants, first_row: int = 0):
        """update_wants with the rows as a bit mask (uint64 words; bit j of word w is row
        first_row + 64 w + j) and the values packed in ascending row order."""
        mask, wants = _c(mask, np.uint64), _c(wants, np.float64)
        self._chk(self._L.dm_store_update_wants_mask(self._ctx, int(first_row), len(mask), _ptr(mask), len(wants),
                                                     _ptr(wants)))

    def apply(self, wants_mask=None, wants=None, release_rows=None, upsert=None, wants_first_row: int = 0,
              now_ns: int | None = None, asynchronous: bool = False):
        """dm_store_apply: one round's refresh (row mask + packed wants), departures and
        arrivals (upsert = (rows, has, wants, subclients, expiry_ns)) in one call.
        Narrow arrivals: has None (= 0), subclients as int32 (sent as 4 B), expiry_ns None
        (= now_ns + the resource's lease length: now_ns is then required).
        asynchronous: dm_store_apply_async -- enqueued, not waited for; the arrays are kept
        alive here until the batch is retired (apply_wait, or two batches later), and a
        rejected batch raises from the call that retires it."""
        b, keep = _fill_batch(_host_col, wants_mask, wants, release_rows, upsert, wants_first_row, now_ns)
        if not asynchronous:
            self._chk(self._L.dm_store_apply(self._ctx, ctypes.byref(b)))
            return
        self._chk(self._L.dm_store_apply_async(self._ctx, ctypes.byref(b)))
        # the library reads these columns until it retires the batch (at most two
        # batches in flight): keep the last three batches' arrays alive
        self._async_keep = (getattr(self, "_async_keep", []) + [keep])[-3:]

    def apply_wait(self):
        """dm_store_apply_wait: retire every in-flight asynchronous batch (raises for the
        first rejected one)."""
        try:
            self._chk(self._L.dm_store_apply_wait(self._ctx))
        finally:
            self._async_keep = []

    def release(self, rows):
        """Release (store.go:142-151)."""
        rows = _c(rows, np.int64)
        self._chk(self._L.dm_store_release(self._ctx, len(rows), _ptr(rows)))

    def clean(self, now_ns: int, peek: bool = False, want_rows: bool = True) -> dict:
        """Clean (store.go:169-181) on the device (dm_store_clean): every lease that has lapsed
        at now_ns (now_ns > expiry) is released as by release().  Returns released (the
        count), next_expiry_ns (the earliest expiry among the rows still live, DM_NO_EXPIRY
        when none is) and rows (the released rows, ascending; None when want_rows is false:
        read_cleaned fetches them later).  peek: the same report, the store unchanged."""
        res = _lib.CleanResult()
        self._chk(self._L.dm_store_clean(self._ctx, int(now_ns), _lib.DM_CLEAN_PEEK if peek else 0,
                                         ctypes.byref(res)))
        self._cleaned = int(res.released)
        return {"released": int(res.released), "next_expiry_ns": int(res.next_expiry_ns),
                "rows": self.read_cleaned(0, int(res.released)) if want_rows else None}

    def read_cleaned(self, off: int = 0, n: int | None = None) -> np.ndarray:
        """dm_read_cleaned: entries [off, off + n) of the last clean's list of released rows
        (n None: from off to its end)."""
        n = getattr(self, "_cleaned", 0) - off if n is None else n
        rows = np.empty(max(int(n), 0), np.int64)
        self._chk(self._L.dm_read_cleaned(self._ctx, int(off), int(n), _ptr(rows)))
        return rows

    def read_store(self, off: int = 0, n: int | None = None) -> dict:
        n = self.n_leases - off if n is None else n
        out = {"has": np.empty(n), "wants": np.empty(n), "subclients": np.empty(n, np.int64),
               "expiry_ns": np.empty(n, np.int64)}
        self._chk(self._L.dm_read_store(self._ctx, off, n, _ptr(out["has"]), _ptr(out["wants"]),
                                      _ptr(out["subclients"]), _ptr(out["expiry_ns"])))
        return out

    # -- the store from and into device memory (no row over PCIe) --
    _DEV_COLS = (("seg_off", "int64"), ("wants", "float64"), ("has", "float64"), ("subclients", "int64"),
                 ("expiry_ns", "int64"))
    _DEV_AGG = (("agg_count", "int64"), ("agg_sum_has", "float64"), ("agg_sum_wants", "float64"))

    def _device_snapshot(self, snap: dict):
        """The columns of a device snapshot, checked without a context or a library call: each
        by _check_device_col, the row columns of one length, the sums one per resource.
        Returns (n_resources, n_leases, {name: column})."""
        have_agg = snap.get("agg_count") is not None
        cols = {}
        for name, dt in self._DEV_COLS + (self._DEV_AGG if have_agg else ()):
            _check_device_col(name, snap[name], (dt,), "snapshot", self.device)
            cols[name] = snap[name]
        if len(cols["seg_off"]) < 1:
            raise ValueError("seg_off must hold n_resources + 1 offsets")
        R, N = len(cols["seg_off"]) - 1, len(cols["wants"])
        for name, _ in self._DEV_COLS[1:]:
            if len(cols[name]) != N:
                raise ValueError(f"{name} has {len(cols[name])} rows, wants has {N}")
        for name, _ in (self._DEV_AGG if have_agg else ()):
            if len(cols[name]) != R:
                raise ValueError(f"{name} has {len(cols[name])} entries for {R} resources")
        return R, N, cols

    def _torch_ready(self):
        """Before a call that reads or writes torch's memory on the context stream: what
        torch's current stream holds is done (a snapshot's producer; the earlier user of a
        block the caching allocator just handed out)."""
        import torch
        torch.cuda.current_stream(self.device).synchronize()
        return torch

    def load_store_device(self, snap: dict):
        """dm_store_load_device: load_store from columns in this device's memory (the same
        keys; torch CUDA tensors).  Leaves the state load_store would for the same values."""
        R, N, cols = self._device_snapshot(snap)
        torch = self._torch_ready()
        seg_off = torch.as_tensor(cols["seg_off"], device=torch.device("cuda", self.device)).cpu().numpy()
        if N != int(seg_off[-1]):
            raise ValueError(f"the row columns hold {N} rows, seg_off ends at {int(seg_off[-1])}")
        s = _lib.Snapshot()
        s.n_resources, s.n_leases = R, N
        for name, t in cols.items():
            setattr(s, name, t.data_ptr() or None)
        self._chk(self._L.dm_store_load_device(self._ctx, ctypes.byref(s)))
        self.n_resources, self.n_leases = R, N
        self.seg_off = seg_off.astype(np.int64, copy=True)

    def load_device(self, snap: dict):
        """load() with the store's columns in device memory (the configuration stays on the host)."""
        self.load_store_device(snap)
        self.load_config(snap)

    def _device_out(self, torch, n, names, columns):
        dt = {"has": torch.float64, "wants": torch.float64, "gets": torch.float64, "sum_has": torch.float64,
              "sum_wants": torch.float64}
        for k in columns:
            if k not in names:
                raise ValueError(f"unknown column {k!r}: one of {names}")
        dev = torch.device("cuda", self.device)
        out = {k: torch.empty(n, dtype=dt.get(k, torch.int64), device=dev) for k in names if k in columns}
        return out, [out[k].data_ptr() or None if k in out else None for k in names]

    def read_store_device(self, off: int = 0, n: int | None = None, columns=None) -> dict:
        """dm_read_store_device: read_store into torch tensors on this device (columns: a
        subset of has, wants, subclients, expiry_ns; default all)."""
        names = ("has", "wants", "subclients", "expiry_ns")
        n = self.n_leases - off if n is None else n
        torch = self._torch_ready()
        out, ptrs = self._device_out(torch, max(int(n), 0), names, names if columns is None else columns)
        self._chk(self._L.dm_read_store_device(self._ctx, int(off), int(n), *ptrs))
        return out

    def store_sums_device(self, r0: int = 0, n: int | None = None, columns=None) -> dict:
        """dm_read_store_sums_device: the store's running sums (count, sum_has, sum_wants: what
        a load takes as agg_*) as torch tensors on this device."""
        names = ("count", "sum_has", "sum_wants")
        n = self.n_resources - r0 if n is None else n
        torch = self._torch_ready()
        out, ptrs = self._device_out(torch, max(int(n), 0), names, names if columns is None else columns)
        self._chk(self._L.dm_read_store_sums_device(self._ctx, int(r0), int(n), *ptrs))
        return out

    def leases_device(self, off: int = 0, n: int | None = None):
        """dm_read_leases_device: leases() as (gets, expiry_ns) torch tensors on this device."""
        names = ("gets", "expiry_ns")
        n = self.n_leases - off if n is None else n
        torch = self._torch_ready()
        out, ptrs = self._device_out(torch, max(int(n), 0), names, names)
        self._chk(self._L.dm_read_leases_device(self._ctx, int(off), int(n), *ptrs))
        return out["gets"], out["expiry_ns"]

    def clone_store_to(self, other: "Engine"):
        """The store, running sums included, into `other` (an engine on the same device)
        without a row leaving HBM: the two store reads into device tensors, then
        other.load_store_device with the sums carried."""
        if other.device != self.device:
            raise ValueError(f"clone_store_to: the other engine is on device {other.device}, this one on {self.device}")
        st = self.read_store_device()
        sums = self.store_sums_device()
        torch = self._torch_ready()
        st["seg_off"] = torch.from_numpy(np.ascontiguousarray(self.seg_off, np.int64)).to(st["has"].device)
        st.update(agg_count=sums["count"], agg_sum_has=sums["sum_has"], agg_sum_wants=sums["sum_wants"])
        other.load_store_device(st)

    # -- store updates from device memory (no column over PCIe) --
    def _device_cols(self, *cols):
        """Update columns in device memory, checked without a context or a library call: cols
        are (name, column, dtype or tuple of dtypes), each checked by _check_device_col and all
        of one length.  Returns that length (0 without columns)."""
        n = None
        for name, t, dts in cols:
            _check_device_col(name, t, (dts,) if isinstance(dts, str) else dts, "update", self.device)
            if n is None:
                n = len(t)
            elif len(t) != n:
                raise ValueError(f"{name} has {len(t)} entries, {cols[0][0]} has {n}")
        return n or 0

    def upsert_device(self, rows, has, wants, subclients, expiry_ns):
        """dm_store_upsert_device: upsert from columns in this device's memory (torch CUDA
        tensors: rows, subclients, expiry_ns int64; has, wants float64), read where they lie."""
        n = self._device_cols(("rows", rows, "int64"), ("has", has, "float64"), ("wants", wants, "float64"),
                              ("subclients", subclients, "int64"), ("expiry_ns", expiry_ns, "int64"))
        self._torch_ready()
        self._chk(self._L.dm_store_upsert_device(self._ctx, n, *[t.data_ptr() or None for t in
                                                                 (rows, has, wants, subclients, expiry_ns)]))

    def update_wants_device(self, rows, wants):
        """dm_store_update_wants_device: update_wants from device columns."""
        n = self._device_cols(("rows", rows, "int64"), ("wants", wants, "float64"))
        self._torch_ready()
        self._chk(self._L.dm_store_update_wants_device(self._ctx, n, rows.data_ptr() or None, wants.data_ptr() or None))

    def update_wants_mask_device(self, mask, wants, first_row: int = 0):
        """dm_store_update_wants_mask_device: update_wants_mask from device columns (the mask's
        words as int64 or uint64 tensors: the bits are what counts)."""
        nw = self._device_cols(("mask", mask, ("int64", "uint64")))
        n = self._device_cols(("wants", wants, "float64"))
        self._torch_ready()
        self._chk(self._L.dm_store_update_wants_mask_device(self._ctx, int(first_row), nw, mask.data_ptr() or None, n,
                                                            wants.data_ptr() or None))

    def release_device(self, rows):
        """dm_store_release_device: release from a device column of rows."""
        n = self._device_cols(("rows", rows, "int64"))
        self._torch_ready()
        self._chk(self._L.dm_store_release_device(self._ctx, n, rows.data_ptr() or None))

    def apply_device(self, wants_mask=None, wants=None, release_rows=None, upsert=None, wants_first_row: int = 0,
                     now_ns: int | None = None, asynchronous: bool = False):
        """dm_store_apply_device: apply() with every column in this device's memory (the mask's
        words int64 or uint64; narrow arrivals: has None, subclients int32, expiry_ns None with
        now_ns).  asynchronous: dm_store_apply_device_async -- the library reads the tensors
        until the batch is retired (apply_wait, or two asynchronous batches later, host or
        device); they are kept alive here until then."""
        # every column is checked before the first pointer is taken (_fill_batch: the now_ns rule first)
        if wants_mask is None and wants is not None:
            raise ValueError("packed wants without a mask")
        for name, t, dts in (("wants_mask", wants_mask, ("int64", "uint64")), ("wants", wants, "float64"),
                             ("release_rows", release_rows, "int64")):
            if t is not None:
                self._device_cols((name, t, dts))
        if upsert is not None:
            rows, has, wv, sub, exp = upsert
            cols = [("upsert rows", rows, "int64"), ("upsert wants", wv, "float64"),
                    ("upsert subclients", sub, ("int64", "int32"))]
            cols += [("upsert has", has, "float64")] if has is not None else []
            cols += [("upsert expiry_ns", exp, "int64")] if exp is not None else []
            self._device_cols(*cols)
        b, keep = _fill_batch(_device_col, wants_mask, wants, release_rows, upsert, wants_first_row, now_ns)
        self._torch_ready()
        if not asynchronous:
            self._chk(self._L.dm_store_apply_device(self._ctx, ctypes.byref(b)))
            return
        self._chk(self._L.dm_store_apply_device_async(self._ctx, ctypes.byref(b)))
        self._async_keep = (getattr(self, "_async_keep", []) + [keep])[-3:]

    def refresh_wants_device(self, wants, first_row: int = 0) -> int:
        """dm_store_refresh_wants_device: wants[i] becomes the wants of row first_row + i
        wherever that row is not released and the value's bits differ from the stored ones
        (a float64 tensor on this device; first_row a multiple of 64).  Returns the number of
        rows written."""
        n = self._device_cols(("wants", wants, "float64"))
        self._torch_ready()
        changed = ctypes.c_int64(0)
        self._chk(self._L.dm_store_refresh_wants_device(self._ctx, int(first_row), n, wants.data_ptr() or None,
                                                        ctypes.byref(changed)))
        return int(changed.value)

    # -- the batch algorithm --
    def apportion(self, now_ns: int, writeback: bool = False, recompute: bool = False, asynchronous: bool = False,
                  wb_columns: str = "auto", defer_join: bool = False):
        """wb_columns: "auto", "inplace" or "alternate" (DM_WB_INPLACE / DM_WB_ALTERNATE);
        defer_join (with asynchronous): DM_DEFER_JOIN."""
        flags = ((_lib.DM_WRITEBACK if writeback else 0) | (_lib.DM_AGG_RECOMPUTE if recompute else 0)
                 | (_lib.DM_ASYNC if asynchronous else 0) | (_lib.DM_DEFER_JOIN if defer_join else 0)
                 | {"auto": 0, "inplace": _lib.DM_WB_INPLACE, "alternate": _lib.DM_WB_ALTERNATE}[wb_columns])
        self._chk(self._L.dm_apportion(self._ctx, int(now_ns), flags))

    def decide(self, now_ns: int, rows, has, wants, subclients):
        """dm_decide: Resource.Decide for each request of a round, in order, each seeing
        the Assigns of the requests before it on its resource (rows[k] = the client's
        row, or a free row of its resource for a new client; a row may repeat);
        returns (gets, expiry_ns).  The device store is not changed."""
        rows = _c(rows, np.int64)
        a = [_c(has, np.float64), _c(wants, np.float64), _c(subclients, np.int64)]
        gets, exp = np.empty(len(rows)), np.empty(len(rows), np.int64)
        self._chk(self._L.dm_decide(self._ctx, int(now_ns), len(rows), _ptr(rows), *[_ptr(x) for x in a], _ptr(gets),
                                    _ptr(exp)))
        return gets, exp

    def decide_assign(self, now_ns: int, rows, has, wants, subclients, safe: bool = False):
        """dm_decide_assign: decide() ended with the Assign (store.go:153-167): each distinct
        requested row takes its last request's (gets, wants, subclients, expiry_ns), as
        decide() followed by that upsert() leaves the store.  Returns (gets, expiry_ns), and
        with safe also each request's safe capacity after the round's Assigns
        (resource.go:81-96): (gets, expiry_ns, safe_capacity)."""
        rows = _c(rows, np.int64)
        a = [_c(has, np.float64), _c(wants, np.float64), _c(subclients, np.int64)]
        gets, exp = np.empty(len(rows)), np.empty(len(rows), np.int64)
        sc = np.empty(len(rows)) if safe else None
        self._chk(self._L.dm_decide_assign(self._ctx, int(now_ns), len(rows), _ptr(rows), *[_ptr(x) for x in a],
                                           _ptr(gets), _ptr(exp), _ptr(sc)))
        return (gets, exp, sc) if safe else (gets, exp)

    def leases(self, off: int = 0, n: int | None = None):
        n = self.n_leases - off if n is None else n
        gets, exp = np.empty(n), np.empty(n, np.int64)
        self._chk(self._L.dm_read_leases(self._ctx, off, n, _ptr(gets), _ptr(exp)))
        return gets, exp

    def leases_rows(self, rows):
        """dm_read_leases_rows: the last tick's leases of scattered rows (gathered on the device)."""
        rows = _c(rows, np.int64)
        gets, exp = np.empty(len(rows)), np.empty(len(rows), np.int64)
        self._chk(self._L.dm_read_leases_rows(self._ctx, len(rows), _ptr(rows), _ptr(gets), _ptr(exp)))
        return gets, exp

    def leases_proto(self, off: int = 0, n: int | None = None):
        n = self.n_leases - off if n is None else n
        cap, exp, ref = np.empty(n), np.empty(n, np.int64), np.empty(n, np.int64)
        self._chk(self._L.dm_read_leases_proto(self._ctx, off, n, _ptr(cap), _ptr(exp), _ptr(ref)))
        return cap, exp, ref

    def resources(self, r0: int = 0, n: int | None = None, safe: bool = True) -> dict:
        n = self.n_resources - r0 if n is None else n
        out = {"count": np.empty(n, np.int64), "sum_has": np.empty(n), "sum_wants": np.empty(n)}
        if safe:
            out["safe_capacity"] = np.empty(n)
        self._chk(self._L.dm_read_resources(self._ctx, r0, n, _ptr(out["count"]), _ptr(out["sum_has"]),
                                          _ptr(out["sum_wants"]), _ptr(out.get("safe_capacity"))))
        return out

    def config(self, r0: int = 0, n: int | None = None) -> dict:
        """dm_read_config: the per-resource configuration the device holds (CFG_FIELDS columns)."""
        n = self.n_resources - r0 if n is None else n
        out = {"kind": np.empty(n, np.int32), "capacity": np.empty(n), "lease_length_s": np.empty(n, np.int64),
               "refresh_interval_s": np.empty(n, np.int64), "learning_end_ns": np.empty(n, np.int64),
               "parent_expiry_ns": np.empty(n, np.int64), "safe_capacity": np.empty(n)}
        self._chk(self._L.dm_read_config(self._ctx, r0, n, *[_ptr(out[k]) for k in CFG_FIELDS]))
        return out

    def publish_totals(self, dev_ptr: int):
        """{SumWants, Count} per resource into a 16 B x R device buffer (server.go:234-255)."""
        self._chk(self._L.dm_publish_totals(self._ctx, ctypes.c_void_p(dev_ptr)))

    # -- profiling --
    def set_profiling(self, on: bool):
        self._chk(self._L.dm_set_profiling(self._ctx, 1 if on else 0))

    def keep_keys(self, on):
        """dm_keep_keys: a wants refresh without NaN keeps the fixed-point keys of every resource
        in which it changed no row's wants bits (off by default).  `on` is a bit set: True or
        _lib.DM_KEEP_REFRESH (1) is that mode; with _lib.DM_KEEP_UPDATES (2) release, upsert and
        the synchronous apply keep the keys of the resources whose rows they did not write; with
        _lib.DM_KEEP_FREE_SLOTS (4) a dense resource that holds released rows (free slots) runs in
        the steady, fixed-point, sweep and cycle forms and keeps a key (plan_info's
        "masked_parts").  No bit changes what a reader sees."""
        self._chk(self._L.dm_keep_keys(self._ctx, int(on)))

    def keep_stats(self) -> dict:
        """dm_keep_stats: the mode and what the context kept under it."""
        arr = (ctypes.c_int64 * 6)()
        self._chk(self._L.dm_keep_stats(self._ctx, arr, 6))
        names = ("mode", "kept_refreshes", "kept_releases", "kept_upserts", "kept_batches", "kept_update_rows")
        return {k: int(arr[i]) for i, k in enumerate(names)}

    def kernel_times(self) -> dict:
        cap = 64
        arr = (_lib.KernelTime * cap)()
        n = self._chk(self._L.dm_kernel_times(self._ctx, arr, cap))
        if n > cap:
            raise RuntimeError(f"dm_kernel_times reports {n} kernel classes, more than {cap}")
        return {arr[i].name.decode(): (arr[i].launches, arr[i].total_ms) for i in range(n) if arr[i].launches}

    def reset_kernel_times(self):
        self._chk(self._L.dm_reset_kernel_times(self._ctx))

    def plan_info(self) -> dict:
        arr = (ctypes.c_int64 * 32)()
        n = self._chk(self._L.dm_plan_info(self._ctx, arr, 32))
        return {_PLAN_NAMES[i]: int(arr[i]) for i in range(min(n, len(_PLAN_NAMES)))}

    def store_lost(self) -> bool:
        """dm_store_lost: a device-side invariant failed; ticks and updates refuse the store
        until it is reloaded, the read calls still work on it."""
        v = ctypes.c_int(0)
        self._chk(self._L.dm_store_lost(self._ctx, ctypes.byref(v)))
        return bool(v.value)

    def store_stats(self) -> dict:
        """dm_store_stats: dense resources (read at 24 B per lease) and their rows,
        resources that may hold explicit expiries, resources, and the workgroup-bin resources
        whose fixed-point key is valid in a part whose keys are in use (their next in-place
        tick loads no row of them while their capacity and kind stay; in a part in the cycle
        form: whose two-tick proof holds), and those of them whose record alternates between
        two running sums (a cycle of period two that is no fixed point)."""
        arr = (ctypes.c_int64 * 6)()
        self._chk(self._L.dm_store_stats(self._ctx, arr, 6))
        return {"dense_resources": int(arr[0]), "dense_leases": int(arr[1]), "explicit_resources": int(arr[2]),
                "resources": int(arr[3]), "fixed_items": int(arr[4]), "cycling_items": int(arr[5])}


def device_count() -> int:
    n = ctypes.c_int()
    rc = lib().dm_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def aggregate_bands(wants, num_clients):
    """GetServerCapacity band sums (server.go:850-868); DmError(DM_E_ARGUMENT) if num_clients < 1."""
    w, nc = _c(wants, np.float64), _c(num_clients, np.int64)
    wt, st = ctypes.c_double(), ctypes.c_int64()
    check(lib().dm_aggregate_bands(_ptr(w), _ptr(nc), len(w), ctypes.byref(wt), ctypes.byref(st)))
    return wt.value, st.value
