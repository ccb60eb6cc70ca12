"""ctypes binding of ``libalphadia_hip.so`` (the C ABI in include/alphadia_hip.h).

Every export is declared once, by ``_abi.declare`` from ``_abi.PROTOTYPES``; the calls below pass plain Python
numbers, ``_p(array, ctype)`` pointers and ``C.byref`` out-parameters, and ctypes converts and checks them.

There is deliberately no fallback: importing this module without the built
library, or creating a context without a GPU, raises.
"""

from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

from alphadia_amd import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADH_LIB_PATH") or os.path.join(_HERE, "libalphadia_hip.so")  # (developer switch: an experimental build)

EXPORTED_SYMBOLS = list(_abi.PROTOTYPES)  # every export of include/alphadia_hip.h, in the header's order


def _process_start_time(pid: str | int = "self") -> float:
    """Wall-clock start of process ``pid`` (this process by default); falls back to now.  Never in the future:
    where /proc/uptime is virtualised (lxcfs) but the start ticks of /proc/<pid>/stat count from the host's
    boot, the difference is meaningless and the result is clamped to the current time."""
    import time

    now = time.time()
    try:
        with open(f"/proc/{pid}/stat") as f:
            ticks = float(f.read().rsplit(")", 1)[1].split()[19])
        with open("/proc/uptime") as f:
            uptime = float(f.read().split()[0])
        return min(now - (uptime - ticks / os.sysconf("SC_CLK_TCK")), now)
    except (OSError, ValueError, IndexError):
        return now


_PROCESS_T0 = _process_start_time()


def _attempt_lower_bound() -> float:
    """Earliest wall-clock time at which rank 0 of THIS attempt can have written the id file.

    Under a launcher (torchrun, mpirun, a script) every rank is a child of the launcher process, whose pid and
    start time are part of the nonce: nothing written before the launcher started can belong to this launch,
    and a rank that starts late (staggered ranks, a slow import) still accepts what rank 0 wrote long before.
    Ranks started by hand with a shared ``ADH_RUN_NONCE`` have a parent (the shell) that outlives the run; there
    the bound is this rank's own start minus ``ADH_RENDEZVOUS_STAGGER_S`` (default 600 s) - pick a new nonce
    per run, a file left by a crashed run of the same nonce inside that window would be accepted."""
    if os.environ.get("ADH_RUN_NONCE"):
        return _PROCESS_T0 - float(os.environ.get("ADH_RENDEZVOUS_STAGGER_S", "600"))
    return min(_process_start_time(os.getppid()), _PROCESS_T0)


class HipBackendError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    _abi.declare(lib)
    _abi.declare(lib, _abi.LFQ_EXPORTS)
    _abi.declare(lib, _abi.FLATTEN_EXPORTS)
    return lib


lib = _load()
_p = _abi.ptr  # (array, ctype) -> the POINTER(ctype) argument of a native call; None stays NULL


def host_threads(n_rows: int) -> tuple[int, int]:
    """(threads a scoring call over ``n_rows`` candidates starts on the host, CPU budget of this process): the
    library's ``adh_host_threads`` - cgroup quota, affinity mask, hardware threads; the rank's share of them."""
    t, b = C.c_int32(0), C.c_int32(0)
    _check(lib.adh_host_threads(int(n_rows), C.byref(t), C.byref(b)), "adh_host_threads")
    return int(t.value), int(b.value)


def chunk_cuts(n_rows: int, ion_mobility: bool = False, max_rows: int = 0, packed: bool = False) -> list[int]:
    """Chunk boundaries of a host -> host scoring call over ``n_rows`` candidates (the library's ``adh_chunk_cuts``):
    chunk i is rows [cuts[i], cuts[i + 1]).  ``max_rows``: the call's bound on a chunk's rows (0: none); ``packed``:
    the compacted copy-out of the padded tables is in use.  Reads the ``ADH_CHUNK*`` switches; needs no GPU."""
    args = (int(n_rows), int(ion_mobility), int(max_rows), int(packed))
    count = C.c_int64(0)
    lib.adh_chunk_cuts(*args, None, 0, C.byref(count))  # (the size query)
    cuts = (C.c_int64 * max(count.value, 1))()
    _check(lib.adh_chunk_cuts(*args, cuts, len(cuts), C.byref(count)), "adh_chunk_cuts")
    return list(cuts[: count.value])


def im_launch_routes(caps: dict, n_class: dict, cfg) -> dict:
    """The library's ``adh_im_launch_routes``: {plan class: (layout, launch)} of an ion-mobility launch with the maxima
    ``caps`` (k, o, s, f and the isotopes i) and ``n_class`` candidates per plan class, for every class that holds any -
    the rule the launches follow.  ``cfg``: a scoring config, or one ``_abi.pack_config`` packed already.  Reads the
    ``ADH_DEBUG_IM*`` switches; needs no GPU."""
    counts = (C.c_int64 * _abi.N_PLAN_CLASSES)()
    for cls, n in n_class.items():
        counts[cls] = int(n)
    layout, launch = (C.c_int32 * _abi.N_PLAN_CLASSES)(), (C.c_int32 * _abi.N_PLAN_CLASSES)()
    packed = cfg if isinstance(cfg, _abi.ScoringConfig) else _abi.pack_config(cfg)
    _check(lib.adh_im_launch_routes(*(int(caps[a]) for a in "kosfi"), counts, C.byref(packed), layout, launch),
           "adh_im_launch_routes")
    return {c: (_abi.IM_LAYOUTS[layout[c]], _abi.IM_LAUNCHES[launch[c]]) for c in range(_abi.N_PLAN_CLASSES) if layout[c]}


_pylib = None       # the same library through ctypes.PyDLL: calls keep the GIL (adh_host_take_objects needs that)
_OBJ_TAKE = None    # None: not probed yet; True / False: the threaded object gather is usable


def _probe_take_objects() -> bool:
    """Is ``ob_refcnt`` the first word of an object here (CPython <= 3.11, no trace-refs build)?  Checked on a probe
    object: five references more after a gather of five, and the gathered entries are the object."""
    global _pylib
    import sys

    if sys.implementation.name != "cpython" or sys.version_info[:2] > (3, 11) or os.environ.get("ADH_NO_OBJECT_TAKE"):
        return False
    #  the gather writes ``ob_refcnt`` as the first word of an object: debug and trace-refs builds put two
    # list pointers in front of it, and free-threaded builds keep the count elsewhere - refuse them by their build
    # flags, not only by the probe below
    import sysconfig

    if (sysconfig.get_config_var("Py_DEBUG") or sysconfig.get_config_var("Py_TRACE_REFS")
            or sysconfig.get_config_var("Py_GIL_DISABLED") or hasattr(sys, "gettotalrefcount")):
        return False
    try:
        _pylib = C.PyDLL(LIB_PATH)
        _abi.declare(_pylib)
        probe = object()
        src = np.empty(1, dtype=object)
        src[0] = probe
        idx = np.zeros(5, dtype=np.int64)
        dst = np.empty(5, dtype=object)
        before = sys.getrefcount(probe)
        rc = _pylib.adh_host_take_objects(_p(dst, C.c_void_p), _p(src, C.c_void_p), _p(idx, C.c_int64), 5, 1, id(None), 1)
        after = sys.getrefcount(probe)
        return rc == 0 and after - before == 5 and all(o is probe for o in dst)
    except Exception:
        return False


def take_objects(src: np.ndarray, idx: np.ndarray, threads: int = 8) -> np.ndarray:
    """``src[idx]`` for a 1-d object array: on several threads through ``adh_host_take_objects`` where that is safe
    (see there), NumPy's own gather otherwise (small inputs, other interpreters, negative indices).

    The call keeps the GIL for its whole duration (``ctypes.PyDLL``: the C threads touch reference counts): Python-level
    code of other threads - the fragments frame's worker, the futures of the host pool when they finish a NumPy call -
    waits meanwhile; only work already inside a GIL-free NumPy loop runs beside it.  ``ADH_NO_OBJECT_TAKE=1`` switches
    it off."""
    global _OBJ_TAKE
    src = np.asarray(src)
    if src.dtype != object or src.ndim != 1 or len(idx) < 262144 or not src.flags.c_contiguous:
        return src[idx]
    if _OBJ_TAKE is None:
        _OBJ_TAKE = _probe_take_objects()
    if not _OBJ_TAKE:
        return src[idx]
    idx64 = np.ascontiguousarray(idx, dtype=np.int64)
    dst = np.empty(len(idx64), dtype=object)
    rc = _pylib.adh_host_take_objects(_p(dst, C.c_void_p), _p(src, C.c_void_p), _p(idx64, C.c_int64), len(idx64), len(src),
                                      id(None), int(threads))
    if rc != 0:  # (an index NumPy would wrap or reject: let NumPy decide; entries written so far are dropped with dst)
        return src[idx]
    return dst


def notnull_objects(a) -> np.ndarray:
    """``pd.notna`` of a 1-d object column of strings and ``None`` (a ``pg`` column) without a Python call per element:
    ``adh_mbr_notnull_objects`` tells ``None`` and ``str`` apart by pointer, pandas is asked about every other entry.
    Where the object layout is not the probed one (see ``_probe_take_objects``), pandas does all of it."""
    global _OBJ_TAKE
    import pandas as pd

    a = np.asarray(a)
    if a.dtype != object or a.ndim != 1 or not a.flags.c_contiguous:
        return np.asarray(pd.notna(a))
    if _OBJ_TAKE is None:
        _OBJ_TAKE = _probe_take_objects()
    if not _OBJ_TAKE:
        return np.asarray(pd.notna(a))
    out, other = np.empty(len(a), np.uint8), C.c_int64(0)
    _check(lib.adh_mbr_notnull_objects(_p(a, C.c_void_p), len(a), id(None), id(str), _p(out, C.c_uint8),
                                       C.byref(other)), "adh_mbr_notnull_objects")
    if other.value:
        rest = np.flatnonzero(out == 2)
        out[rest] = pd.notna(a[rest])
    return out.view(np.bool_)


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib.adh_last_error()
        raise HipBackendError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def table_layout(rows: int, top_k: int) -> tuple[list[dict], int, int]:
    """``adh_table_layout``: the packed device buffer of ``rows`` candidates as the library lays it out -
    (fields in buffer order, total bytes, bytes of the wire prefix).  Needs no GPU."""
    n = C.c_int32(0)
    total, wire = C.c_uint64(0), C.c_uint64(0)
    _check(lib.adh_table_layout(int(rows), int(top_k), 0, None, C.byref(n), C.byref(total), C.byref(wire)),
           "adh_table_layout")
    arr = (_abi.TableField * n.value)()
    _check(lib.adh_table_layout(int(rows), int(top_k), n.value, arr, C.byref(n), C.byref(total), C.byref(wire)),
           "adh_table_layout")
    fields = [dict(name=f.name.decode(), offset=int(f.offset), row_elems=int(f.row_elems), elem_bytes=int(f.elem_bytes),
                   wire=bool(f.wire)) for f in arr]
    return fields, int(total.value), int(wire.value)


def trim_device_cache() -> None:
    """``adh_trim_device_cache``: give the device buffers the library keeps parked back to the runtime."""
    _check(lib.adh_trim_device_cache(), "adh_trim_device_cache")


def device_count() -> int:
    n = C.c_int(0)
    _check(lib.adh_device_count(C.byref(n)), "adh_device_count")
    return n.value


class PinnedPool:
    """Page-locked host buffers (``adh_host_alloc``) handed out as numpy arrays and reused by tag.

    H2D / D2H copies from page-locked memory run asynchronously at the full PCIe rate; allocating
    it is slow (it pins pages), hence the pool: a buffer is grown, never shrunk, and the array
    returned for a tag is only valid until the same tag is requested again."""

    def __init__(self):
        self._bufs: dict[str, tuple[int, int]] = {}

    def empty(self, tag: str, shape, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        ptr, cap = self._bufs.get(tag, (0, 0))
        if cap < nbytes or ptr == 0:
            if ptr:
                lib.adh_host_free(ptr)
                self._bufs.pop(tag, None)
            want = max(nbytes + nbytes // 8, 64)
            p = C.c_void_p()
            _check(lib.adh_host_alloc(C.byref(p), want), "adh_host_alloc")
            ptr, cap = int(p.value), want
            self._bufs[tag] = (ptr, cap)
        if nbytes == 0:
            return np.empty(shape, dtype=dtype)
        raw = (C.c_uint8 * nbytes).from_address(ptr)
        return np.frombuffer(raw, dtype=dtype).reshape(shape)

    def take(self, tag: str, src: np.ndarray, order: np.ndarray | None = None, dtype=None) -> np.ndarray:
        """``src[order]`` (or a copy of ``src``) written straight into the pooled buffer of ``tag``."""
        src = np.asarray(src)
        dtype = np.dtype(dtype or src.dtype)
        if order is None:
            out = self.empty(tag, src.shape, dtype)
            out[...] = src
            return out
        out = self.empty(tag, (len(order),) + src.shape[1:], dtype)
        if src.dtype == dtype and out.size:
            np.take(src, order, axis=0, out=out)
        elif out.size:
            out[...] = src[order]
        return out

    def close(self):
        for ptr, _ in self._bufs.values():
            lib.adh_host_free(ptr)
        self._bufs.clear()


def _launch_nonce() -> bytes:
    """What all ranks of ONE launch share and a later launch does not: the launcher process (parent of every
    rank) and its start time, plus whatever the launcher exports.  ``ADH_RUN_NONCE`` overrides (ranks started
    by hand from one shell share a parent that outlives the run)."""
    import hashlib

    ppid = os.getppid()
    start = ""
    try:
        with open(f"/proc/{ppid}/stat") as f:
            start = f.read().rsplit(")", 1)[1].split()[19]  # field 22: start time of the process
    except (OSError, IndexError):
        pass
    # (the restart count: an elastic restart under the same launcher is a new attempt with a new id file)
    tag = "|".join([os.environ.get("ADH_RUN_NONCE", ""), os.environ.get("MASTER_PORT", "0"),
                    os.environ.get("TORCHELASTIC_RUN_ID", "none"), os.environ.get("TORCHELASTIC_RESTART_COUNT", "0"),
                    str(ppid), start])
    return hashlib.sha256(tag.encode()).digest()


def _proc_start_ticks(pid: int) -> int:
    """Start time of process ``pid`` in clock ticks since boot (field 22 of /proc/<pid>/stat); -1 when it is gone."""
    try:
        with open(f"/proc/{pid}/stat") as f:
            return int(f.read().rsplit(")", 1)[1].split()[19])
    except (OSError, IndexError, ValueError):
        return -1


def _writer_tag(pid: int) -> bytes:
    """16 bytes that name the process that wrote an id file: pid and its start time (a recycled pid differs in the latter)."""
    import struct

    return struct.pack("<qq", int(pid), _proc_start_ticks(pid))


def _writer_alive(tag: bytes) -> bool:
    import struct

    pid, start = struct.unpack("<qq", tag)
    return pid > 0 and start >= 0 and _proc_start_ticks(pid) == start


_EXIT_REMOVALS: list = []


def _remove_at_exit(path: str) -> None:
    import atexit

    if not _EXIT_REMOVALS:
        def _cleanup():
            for p, tag in _EXIT_REMOVALS:
                try:  # (only a file this process wrote: a later attempt may have replaced it)
                    with open(p, "rb") as f:
                        data = f.read()
                    if data[32:48] == tag:
                        os.remove(p)
                except OSError:
                    pass

        atexit.register(_cleanup)
    _EXIT_REMOVALS.append((path, _writer_tag(os.getpid())))


def rendezvous_path() -> str:
    if os.environ.get("ADH_RENDEZVOUS_FILE"):
        return os.environ["ADH_RENDEZVOUS_FILE"]
    base = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    folder = os.path.join(base, f"adh_{os.getuid()}")  # a directory of this user only: nobody else can pre-create
    os.makedirs(folder, mode=0o700, exist_ok=True)      # or redirect the id file
    import stat as _stat

    st = os.lstat(folder)  # (not stat: a planted symlink to some other private directory of the user must not pass)
    if not _stat.S_ISDIR(st.st_mode) or st.st_uid != os.getuid() or (st.st_mode & 0o077):
        raise HipBackendError(f"{folder} is not a private directory of this user")
    return os.path.join(folder, f"rccl_id_{_launch_nonce().hex()[:24]}")


def rendezvous_unique_id(rank: int, world: int, timeout: float = 300.0, make_id=None) -> bytes:
    """Hand rank 0's RCCL unique id to the other ranks of THIS NODE through a file in /dev/shm.

    The file is named after a per-launch nonce (launcher pid + start time, MASTER_PORT, run id) and starts
    with that nonce; rank 0 removes whatever a crashed earlier launch left under the name, creates the file
    exclusively (0600, inside a 0700 directory of this user) and removes it again once the communicator exists
    (``Context.comm_init``); readers only accept a file that carries their own nonce.  Single node: the ranks
    must share a file system and a launcher (checked through LOCAL_WORLD_SIZE)."""
    import time

    local_world = os.environ.get("LOCAL_WORLD_SIZE")
    if local_world is not None and int(local_world) != int(world):
        raise HipBackendError("the RCCL id rendezvous goes through a node-local file: all ranks must run on one node "
                              f"(WORLD_SIZE {world}, LOCAL_WORLD_SIZE {local_world})")
    path = rendezvous_path()
    nonce = _launch_nonce()
    if rank == 0:
        if make_id is None:
            buf = C.create_string_buffer(128)
            _check(lib.adh_comm_unique_id(buf), "adh_comm_unique_id")
            uid = buf.raw
        else:
            uid = bytes(make_id())
        try:
            os.unlink(path)  # a stale file of a crashed launch with the same nonce inputs
        except FileNotFoundError:
            pass
        tmp = f"{path}.{os.getpid()}.tmp"
        fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_EXCL, 0o600)
        with os.fdopen(fd, "wb") as f:
            f.write(nonce + _writer_tag(os.getpid()) + uid)
        os.replace(tmp, path)  # atomic: readers see all of it or nothing
        _remove_at_exit(path)  # (a rank 0 that fails before Context.comm_init removes the file still cleans up)
        return uid
    t0 = time.time()
    while True:
        try:
            with open(path, "rb") as f:
                data = f.read()
                written = os.fstat(f.fileno()).st_mtime
            # a file older than the launch is what an earlier attempt with the same nonce inputs left behind
            # (rank 0 replaces it); the bound is the LAUNCHER's start, not this rank's: ranks may start seconds
            # or minutes apart (_attempt_lower_bound)
            fresh = written >= _attempt_lower_bound() - 2.0
            if fresh and len(data) == len(nonce) + 16 + 128 and data[: len(nonce)] == nonce:
                # ... and a file whose writer is gone is what a crashed attempt of THIS launch left (same launcher,
                # same port, seconds ago): rank 0 is alive while its peers read - it waits for them inside
                # ncclCommInitRank - so a dead writer means "not this attempt's"; the new rank 0 replaces the file
                if _writer_alive(data[len(nonce): len(nonce) + 16]):
                    return data[len(nonce) + 16:]
        except FileNotFoundError:
            pass
        if time.time() - t0 > timeout:
            raise HipBackendError(f"rank {rank}: no RCCL unique id at {path} after {timeout:.0f} s")
        time.sleep(0.01)


class Context:
    """One GPU: staged run + library + candidate table (an ``adh_handle_t``)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib.adh_create(C.byref(self._h), device), "adh_create")
        self.device = device
        self._run_key = None
        self._lib_key = None
        self.n_candidates = 0
        self.pinned = PinnedPool()
        self.comm_world = 1
        self.comm_rank = 0
        # one more per scoring call that replaces the device tables (a resident result checks it is still current)
        self.tables_serial = 0
        # ... and one more per selection or staging call (a resident selection checks it is still current)
        self.select_serial = 0
        self._sessions = weakref.WeakSet()  # the live _DeviceSession objects of this handle

    def _close_sessions(self):
        """Destroy every live session while the handle still exists: a session's native destroy reads the handle's
        device and stream, and one that outlived the handle could only leak its device memory."""
        for s in list(self._sessions):
            s.close()

    def close(self):
        if self._h:
            self._close_sessions()
            lib.adh_destroy(self._h)
            self._h = C.c_void_p()
            self.pinned.close()

    # -- multi-GPU (one process per GPU; RCCL behind the C ABI) -------------
    def comm_init(self, rank: int, world: int, max_rows_per_rank: int, unique_id: bytes | None = None,
                  timeout: float = 600.0) -> None:
        """Attach an RCCL communicator: every later ``score_host`` also all-gathers the computed
        tables of all ranks into HBM (``gathered_tables``).  Creating the communicator is collective; a rank
        whose peers never arrive (e.g. a stale unique id) fails after ``timeout`` seconds instead of hanging."""
        import threading

        uid = unique_id if unique_id is not None else rendezvous_unique_id(rank, world)
        buf = C.create_string_buffer(bytes(uid), 128)
        result: list = []

        def call():
            result.append(lib.adh_comm_init(self._h, rank, world, buf, int(max_rows_per_rank)))
            msg = lib.adh_last_error()  # (thread-local: fetched on the thread that made the call)
            result.append(msg.decode() if msg else "")

        t = threading.Thread(target=call, name="adh_comm_init", daemon=True)
        t.start()
        t.join(timeout)
        if t.is_alive():
            raise HipBackendError(f"adh_comm_init: rank {rank} of {world} still waits for its peers after {timeout:.0f} s "
                                  "(ncclCommInitRank is collective: did every rank start, with the same unique id?)")
        if result[0] != 0:
            raise HipBackendError(f"adh_comm_init failed ({result[0]}): {result[1]}")
        self.comm_rank, self.comm_world = int(rank), int(world)
        self._comm_attached = True
        if unique_id is None and rank == 0:
            # communicator creation is collective: every rank has read the id by now
            try:
                os.remove(rendezvous_path())
            except OSError:
                pass

    def comm_destroy(self) -> None:
        _check(lib.adh_comm_destroy(self._h), "adh_comm_destroy")
        self.comm_rank, self.comm_world = 0, 1
        self._comm_attached = False

    def comm_wait(self) -> None:
        _check(lib.adh_comm_wait(self._h), "adh_comm_wait")

    def barrier(self) -> None:
        _check(lib.adh_comm_barrier(self._h), "adh_comm_barrier")

    def all_gather_rows(self, local: np.ndarray, rows_per_rank: list[int]) -> np.ndarray:
        """Concatenation, in rank order, of every rank's ``local`` array (``rows_per_rank[r]`` rows on rank r,
        equal trailing shape and dtype): ``adh_comm_all_gather_host`` with the shards padded to the longest
        one.  With one rank (no communicator) the array comes back as it is."""
        rank, world = self.comm_info()
        if len(rows_per_rank) != world:
            raise ValueError(f"rows_per_rank has {len(rows_per_rank)} entries for {world} ranks")
        local = np.ascontiguousarray(local)
        if local.shape[0] != rows_per_rank[rank]:
            raise ValueError(f"rank {rank} holds {local.shape[0]} rows, rows_per_rank says {rows_per_rank[rank]}")
        if world == 1 and not getattr(self, "_comm_attached", False):
            return local
        cap = max(int(r) for r in rows_per_rank)
        row_bytes = int(np.prod(local.shape[1:], dtype=np.int64)) * local.dtype.itemsize
        send = np.zeros((cap,) + local.shape[1:], dtype=local.dtype)
        send[: local.shape[0]] = local
        recv = np.empty((world, cap) + local.shape[1:], dtype=local.dtype)
        _check(lib.adh_comm_all_gather_host(self._h, _p(send), cap * row_bytes, _p(recv)), "adh_comm_all_gather_host")
        return np.concatenate([recv[r, : int(rows_per_rank[r])] for r in range(world)], axis=0)

    def all_reduce_max(self, value: float) -> float:
        v = C.c_double(float(value))
        _check(lib.adh_comm_all_reduce_max(self._h, C.byref(v)), "adh_comm_all_reduce_max")
        return float(v.value)

    def comm_info(self) -> tuple[int, int]:
        """(rank, world) as RCCL reports them for the attached communicator; (0, 1) without one."""
        r, w = C.c_int(0), C.c_int(1)
        _check(lib.adh_comm_info(self._h, C.byref(r), C.byref(w)), "adh_comm_info")
        return int(r.value), int(w.value)

    def device_synchronize(self) -> None:
        _check(lib.adh_device_synchronize(self._h), "adh_device_synchronize")

    def _view_to_host(self, view: _abi.Output, rows: int, names=None) -> dict:
        out = {}
        for name, (shape, dt) in _abi.output_shapes(rows, int(view.top_k), extras=True).items():
            if names is not None and name not in names:
                continue
            ptr = C.cast(getattr(view, name), C.c_void_p).value
            if not ptr:
                continue
            a = np.empty(shape, dtype=dt)
            _check(lib.adh_copy_to_host(self._h, _p(a), ptr, a.nbytes), "adh_copy_to_host")
            out[name] = a
        return out

    def device_tables(self) -> _abi.Output:
        """Device view of the tables of the last ``score_host`` call (they stay in HBM)."""
        view = _abi.Output()
        _check(lib.adh_get_device_tables(self._h, C.byref(view)), "adh_get_device_tables")
        return view

    def debug_get_dense(self, frame_start, frame_stop, mz_query, mass_tolerance, quad_lo, quad_hi,
                        scan_start: int = 0, scan_stop: int = 1):
        """The gather kernel's dense tile for one query (test entry): ``(dense[2, K, O, S, F], obs)``
        as ``get_dense(..., absolute_masses=True)`` returns them (S = 1 for AlphaRaw runs)."""
        q = _abi.as_c(mz_query, np.float32)
        cap = 2 * q.shape[0] * 8 * max(int(scan_stop) - int(scan_start), 1) * (int(frame_stop) - int(frame_start) + 1)
        buf = np.zeros(max(cap, 1), dtype=np.float32)
        obs = np.zeros(8, dtype=np.int32)
        n_obs, n_s, n_f = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(
            lib.adh_debug_get_dense(
                self._h, int(frame_start), int(frame_stop), int(scan_start), int(scan_stop), _p(q, C.c_float), q.shape[0],
                mass_tolerance, quad_lo, quad_hi, _p(buf, C.c_float), buf.shape[0], _p(obs, C.c_int32), C.byref(n_obs),
                C.byref(n_s), C.byref(n_f)),
            "adh_debug_get_dense",
        )
        K, O, S, F = q.shape[0], n_obs.value, n_s.value, n_f.value
        return buf[: 2 * K * O * S * F].reshape(2, K, O, S, F).copy(), obs[:O].astype(np.int64)

    def debug_log_f32(self, x, lds_table: bool = False):
        """The selection's table-driven log on the device (test entry): ``(out64, out32)`` for the float32 values
        ``x`` - the float64 log where it is defined (1 <= x < inf, NaN elsewhere) and the float32 value the smoothing
        kernels store (their three-way dispatch).  ``lds_table``: read the table from a copy in LDS."""
        x = _abi.as_c(x, np.float32).reshape(-1)
        out64, out32 = np.empty(x.shape[0], np.float64), np.empty(x.shape[0], np.float32)
        _check(lib.adh_debug_log_f32(self._h, _p(x, C.c_float), x.shape[0], int(bool(lds_table)), _p(out64, C.c_double),
                                     _p(out32, C.c_float)), "adh_debug_log_f32")
        return out64, out32

    def debug_log_f32_sweep(self, first_bits: int, last_bits: int, lds_table: bool = False, capacity: int = 4096) -> dict:
        """The same log over every float32 bit pattern in ``[first_bits, last_bits]`` against the device library's
        log (test entry): ``count`` arguments whose float32-rounded logs differ, the first ``capacity`` of them in
        ``bits`` (ascending), and the largest float64 difference ``max_ulps`` at the argument ``max_bits``."""
        for name, v in (("first_bits", first_bits), ("last_bits", last_bits)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} is no 32-bit pattern: {v!r}")
        bits = np.zeros(max(int(capacity), 1), np.uint32)
        count, ulps, at = C.c_int64(0), C.c_double(0.0), C.c_uint32(0)
        _check(lib.adh_debug_log_f32_sweep(self._h, int(first_bits), int(last_bits), int(bool(lds_table)), C.byref(count),
                                           _p(bits, C.c_uint32), int(capacity), C.byref(ulps), C.byref(at)),
               "adh_debug_log_f32_sweep")
        return {"count": int(count.value), "bits": bits[: min(int(count.value), max(int(capacity), 0))].copy(),
                "max_ulps": float(ulps.value), "max_bits": int(at.value)}

    def d2h_bytes(self, reset: bool = False) -> int:
        """Bytes the library copied device -> host on this GPU since the last reset."""
        v = C.c_uint64(0)
        _check(lib.adh_transfer_counters(self._h, C.byref(v), int(reset)), "adh_transfer_counters")
        return int(v.value)

    def fdr_resident(self, mlp: "DeviceMlp", group_a, group_b=None, tiebreak=None, cycle=None,
                     rt_tol_seconds: float = 3.0, mass_tol_ppm: float = 15.0, fdr_heuristic: float = 0.1):
        """fdr.py:134-178 on the device for rows staged with ``DeviceMlp.stage_rows_device`` and scored
        with ``predict_resident``: returns ``(candidate_row, proba, qval)`` of the surviving PSMs."""
        ga = _abi.as_c(group_a, np.int64)
        gb = _abi.as_c(group_b, np.int64) if group_b is not None else None
        tb = _abi.as_c(tiebreak, np.int64) if tiebreak is not None else None
        cyc = _abi.as_c(cycle, np.float64) if cycle is not None else None
        if cyc is not None and (cyc.ndim != 4 or cyc.shape[0] != 1 or cyc.shape[3] != 2):
            raise ValueError("cycle must have shape (1, cycle_len, cycle_scans, 2)")
        m = mlp.n_rows
        rows, proba, qval = np.zeros(m, np.int64), np.zeros(m, np.float32), np.zeros(m, np.float64)
        n_out = C.c_int64(0)
        _check(
            lib.adh_fdr_resident(
                self._h, mlp._s, _p(ga, C.c_int64), _p(gb, C.c_int64), _p(tb, C.c_int64), _p(cyc, C.c_double),
                cyc.shape[1] if cyc is not None else 0, cyc.shape[2] if cyc is not None else 0, rt_tol_seconds,
                mass_tol_ppm, fdr_heuristic, C.byref(n_out), _p(rows, C.c_int64), _p(proba, C.c_float), _p(qval, C.c_double)),
            "adh_fdr_resident",
        )
        k = int(n_out.value)
        return rows[:k], proba[:k], qval[:k]

    def zero_device_tables(self, stream: int = 0) -> None:
        _check(lib.adh_zero_device_tables(self._h, stream), "adh_zero_device_tables")

    def table_rows_to_host(self, name: str, start: int, stop: int) -> np.ndarray:
        """Rows [start, stop) of the device table ``name`` (of the current tables), copied to the host."""
        view = self.device_tables()
        shape, dt = _abi.output_shapes(int(view.n), int(view.top_k), extras=True)[name]
        if not 0 <= start <= stop <= int(view.n):
            raise ValueError(f"rows [{start}, {stop}) outside the {int(view.n)} rows of the device tables")
        row_shape = tuple(shape[1:])
        a = np.empty((stop - start,) + row_shape, dtype=dt)
        ptr = C.cast(getattr(view, name), C.c_void_p).value
        if a.nbytes:
            row_bytes = int(np.prod(row_shape, dtype=np.int64)) * np.dtype(dt).itemsize
            _check(lib.adh_copy_to_host(self._h, _p(a), ptr + start * row_bytes, a.nbytes), "adh_copy_to_host")
        return a

    def device_tables_to_host(self, names=None) -> dict:
        view = self.device_tables()
        return self._view_to_host(view, int(view.n), names)

    def gathered_tables(self, rank: int, rows: int | None = None) -> dict:
        """Host copy of the computed ("wire") tables rank ``rank`` contributed to the last all-gather."""
        view = _abi.Output()
        n = C.c_int64(0)
        _check(lib.adh_comm_gathered(self._h, rank, C.byref(view), C.byref(n)), "adh_comm_gathered")
        return self._view_to_host(view, int(n.value) if rows is None else int(rows))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- staging ---------------------------------------------------------
    @staticmethod
    def _key(*arrays):
        """Identity of host arrays that are staged in HBM: address, shape, dtype and a checksum of a
        strided sample (<= 64 K elements per array).  The arrays themselves are kept alive while they
        are staged (``_run_keepalive`` / ``_lib_keepalive``), so an address cannot be handed to a new
        array; the checksum catches in-place edits."""
        import zlib

        key = []
        for a in map(np.asarray, arrays):
            flat = a.reshape(-1)
            step = max(1, flat.shape[0] // 65536)
            crc = zlib.crc32(np.ascontiguousarray(flat[::step]).view(np.uint8)) if flat.shape[0] else 0
            key.append((a.__array_interface__["data"][0], a.shape, str(a.dtype), crc))
        return tuple(key)

    def stage_run(self, dia, force: bool = False) -> bool:
        """Copy the run to HBM unless this very run is already staged."""
        if hasattr(dia, "tof_indptr"):  # TimsTOFTransposeJIT layout (bruker_jit.py:22-137)
            key = self._key(dia.mz_values, dia.intensity_values, dia.push_indices, dia.tof_indptr)
            if not force and key == self._run_key:
                return False
            m = _abi.pack_timstof(dia)
            self.select_serial += 1
            _check(lib.adh_stage_timstof(self._h, m.ref()), "adh_stage_timstof")
            self._run_key = key
            self._run_keepalive = (dia.mz_values, dia.intensity_values, dia.push_indices, dia.tof_indptr)
            return True
        key = self._key(dia.mz_values, dia.intensity_values, dia.peak_start_idx_list, dia.rt_values)
        if not force and key == self._run_key:
            return False
        m = _abi.pack_alpharaw(dia)
        self.select_serial += 1
        _check(lib.adh_stage_alpharaw(self._h, m.ref()), "adh_stage_alpharaw")
        self._run_key = key
        self._run_keepalive = (dia.mz_values, dia.intensity_values, dia.peak_start_idx_list, dia.rt_values)
        return True

    def stage_fragments(self, *columns, force: bool = False) -> bool:
        key = self._key(*columns)
        if not force and key == self._lib_key:
            return False
        m = _abi.pack_fragments(*columns)
        self.select_serial += 1
        _check(lib.adh_stage_fragments(self._h, m.ref()), "adh_stage_fragments")
        self._staged_library(columns, m.struct.n, key)
        return True

    def _staged_library(self, columns, n: int, key) -> None:
        """Bookkeeping of a staged library: the key of the nine columns it equals (None: no host column set), the key
        of the eight columns it was staged from, the columns themselves (their addresses are part of the keys)."""
        self._lib_key = key
        if key is not None:  # (a key holds one entry per column)
            self._lib_source = key[:1] + key[2:]
        else:
            self._lib_source = self._key(*columns[:1], *columns[2:]) if len(columns) == 9 else self._key(*columns)
        self._lib_keepalive = columns
        self._n_lib = int(n)

    def stage_fragments_columns(self, *columns) -> None:
        """``adh_stage_fragments_columns`` without a model: what ``stage_fragments(*columns, force=True)`` stages, the
        records packed by a kernel from the uploaded columns."""
        m = _abi.pack_fragments(*columns)
        self._lib_key = None
        self.select_serial += 1
        _check(lib.adh_stage_fragments_columns(self._h, m.ref(), None, None), "adh_stage_fragments_columns")
        self._staged_library(columns, m.struct.n, self._key(*columns))

    def stage_fragments_calibrated(self, model, mz_library, intensity, type, loss_type, charge, number, position,  # noqa: A002
                                   cardinality) -> np.ndarray:
        """Stage the library from its eight columns with ``mz`` = float32 of the fitted ``model`` over ``mz_library``,
        evaluated while the records are packed in HBM.  Returns the float64 predictions (the ``mz_calibrated`` column
        of the frame).  The staged library then equals no host column set: ``adopt_fragment_columns`` names one."""
        packed = _abi.pack_loess_model(model.scale_mean, model.scale_max, model.beta)
        columns = (mz_library, intensity, type, loss_type, charge, number, position, cardinality)
        m = _abi.pack_fragments_calibrated(*columns)
        y = np.empty(int(m.struct.n), dtype=np.float64)
        self._lib_key = None
        self.select_serial += 1
        _check(lib.adh_stage_fragments_columns(self._h, m.ref(), C.byref(packed), _p(y, C.c_double)),
               "adh_stage_fragments_columns")
        self._staged_library(columns, m.struct.n, None)
        return y

    def stage_candidate_library(self, tables, model=None):
        """``adh_stage_candidate_library``: build and stage the library of all fragment series of the precursors in
        ``tables`` (a ``Marshalled`` ``adh_candidate_library_t``, ``_abi.pack_candidate_library``) in HBM, with ``mz``
        = float32 of the fitted ``model`` over ``mz_library`` when one is given.  Returns ``(flat_frag_start_idx,
        flat_frag_stop_idx, mz_library, mz_calibrated)``: uint32 per precursor, float32 and float64 (None without a
        model) per row.  The staged library then equals no host column set: ``adopt_fragment_columns`` names one.  A
        refused table leaves the staged library and its bookkeeping as they were."""
        packed = _abi.pack_loess_model(model.scale_mean, model.scale_max, model.beta) if model is not None else None
        st = tables.struct
        n = int(st.n)
        offsets = np.ctypeslib.as_array(st.seq_offset, shape=(n + 1,))
        # (the row count the C side will arrive at, for the output columns; a table it refuses writes nothing)
        total = int((np.diff(offsets) - 1).sum()) * int(st.n_series) if n else 0
        if not 0 <= total < 0xFFFFFFFF or (n and int(np.diff(offsets).min()) < 2):
            total = 0
        start, stop = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        mz_library = np.empty(total, dtype=np.float32)
        y = np.empty(total, dtype=np.float64) if packed is not None else None
        rc = lib.adh_stage_candidate_library(
            self._h, tables.ref(), C.byref(packed) if packed is not None else None, _p(start, C.c_uint32),
            _p(stop, C.c_uint32), _p(mz_library, C.c_float), _p(y, C.c_double))
        if rc in (-1, -4):  # ADH_ERR_INVALID_ARGUMENT, ADH_ERR_UNSUPPORTED: refused before anything was touched
            _check(rc, "adh_stage_candidate_library")
        self._lib_key = None
        self.select_serial += 1
        _check(rc, "adh_stage_candidate_library")
        self._staged_library((mz_library,), total, None)
        return start, stop, mz_library, y

    def calibrate_staged_fragments(self, model) -> np.ndarray:
        """``adh_calibrate_staged_fragments``: rewrite ``mz`` of the staged library, in HBM, as float32 of the fitted
        ``model`` over the staged ``mz_library``.  Returns the float64 predictions.  The staged library then equals
        no host column set (a later ``stage_fragments`` with the old columns stages again) until
        ``adopt_fragment_columns`` names one."""
        packed = _abi.pack_loess_model(model.scale_mean, model.scale_max, model.beta)
        y = np.empty(getattr(self, "_n_lib", 0), dtype=np.float64)  # (no library: the call says so)
        self._lib_key = None
        self.select_serial += 1
        _check(lib.adh_calibrate_staged_fragments(self._h, C.byref(packed), _p(y, C.c_double)),
               "adh_calibrate_staged_fragments")
        return y

    def adopt_fragment_columns(self, *columns) -> None:
        """Declare that the staged library equals these nine host columns (``fragment_columns(df, "mz_calibrated")``
        after the calibrated column was written into the frame): the next ``stage_fragments`` with them skips.
        Copies nothing."""
        if len(columns) != 9:
            raise ValueError("adopt_fragment_columns takes the nine fragment columns")
        n = getattr(self, "_n_lib", None)
        if n is None:
            raise HipBackendError("no fragment library staged")
        if any(np.asarray(c).shape != (n,) for c in columns):
            raise ValueError(f"fragment columns do not have the staged library's {n} rows")
        self._staged_library(columns, n, self._key(*columns))

    def staged_from(self, mz_library, intensity, type, loss_type, charge, number, position, cardinality) -> bool:  # noqa: A002
        """Whether the staged library was staged from these columns: its key matches them in every position but the
        m/z one."""
        source = getattr(self, "_lib_source", None)
        return source is not None and source == self._key(mz_library, intensity, type, loss_type, charge, number,
                                                          position, cardinality)

    def staged_fragment_records(self, host_mirror: bool = False) -> np.ndarray:
        """The raw records of the staged library (``_abi.LIB_RECORD_DTYPE``), from HBM or from the host mirror."""
        out = np.empty(getattr(self, "_n_lib", 0), dtype=_abi.LIB_RECORD_DTYPE)
        _check(lib.adh_staged_fragments_read(self._h, int(bool(host_mirror)), _p(out), out.shape[0]),
               "adh_staged_fragments_read")
        return out

    def flatten_library(self, frag_start, frag_stop, elution_group, decoy, mz, intensity, column_codes, top_k: int,
                        min_intensity: float, stage: bool = False) -> dict:
        """The device flatten (include/alphadia_hip_flatten.h: ``adfl_flatten``): int64 precursor columns (``decoy``
        uint8 or None), the two float32 matrices ``[n_rows, n_cols]`` and ``column_codes[4, n_cols]`` (type,
        loss_type, charge, counts-from-the-N-terminus) in; ``flat_frag_start_idx`` / ``flat_frag_stop_idx`` per
        precursor and the eight flat columns out, with ``routes``, ``kernel_ms`` and the link bytes of the call.
        ``stage``: the records are left staged on this context, as ``stage_fragments_columns`` of the returned
        columns would leave them (``adopt_fragment_columns`` then names them).  A refused input raises ``ValueError``
        and leaves the staged library and its bookkeeping as they were."""
        start, stop, eg = (_abi.as_c(a, np.int64) for a in (frag_start, frag_stop, elution_group))
        dec = _abi.as_c(decoy, np.uint8) if decoy is not None else None
        mz, intensity = _abi.as_c(mz, np.float32), _abi.as_c(intensity, np.float32)
        codes = _abi.as_c(column_codes, np.uint8)
        n = start.shape[0]
        if mz.ndim != 2 or mz.shape != intensity.shape or codes.shape != (4, mz.shape[1]):
            raise ValueError("flatten_library: two matrices of one shape and four codes per column")
        if stop.shape != (n,) or eg.shape != (n,) or (dec is not None and dec.shape != (n,)):
            raise ValueError("flatten_library: precursor columns differ in length")
        n_rows, n_cols = mz.shape
        capacity = int(np.minimum(np.clip(stop - start, 0, 255) * n_cols, max(int(top_k), 0)).sum())
        flat_start, flat_stop = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        out_mz, out_int = np.empty(capacity, dtype=np.float32), np.empty(capacity, dtype=np.float32)
        out_bytes = np.empty((6, capacity), dtype=np.uint8)
        n_flat, routes, ms, link = C.c_int64(0), (C.c_int64 * 4)(), C.c_double(0.0), (C.c_uint64 * 2)()
        rc = lib.adfl_flatten(self._h, n, _p(start, C.c_int64), _p(stop, C.c_int64), _p(eg, C.c_int64), _p(dec, C.c_uint8),
                              n_rows, n_cols, _p(mz, C.c_float), _p(intensity, C.c_float), _p(codes, C.c_uint8), int(top_k),
                              float(min_intensity), int(bool(stage)), capacity, _p(flat_start, C.c_uint32),
                              _p(flat_stop, C.c_uint32), _p(out_mz, C.c_float), _p(out_int, C.c_float),
                              _p(out_bytes, C.c_uint8), C.byref(n_flat), routes, C.byref(ms), link)
        if rc == -1:  # ADH_ERR_INVALID_ARGUMENT: refused before anything was touched
            msg = lib.adh_last_error()
            raise ValueError(msg.decode() if msg else "adfl_flatten refused its input")
        if stage:
            self._lib_key = None
            self.select_serial += 1
        _check(rc, "adfl_flatten")
        k = int(n_flat.value)
        out = dict(flat_frag_start_idx=flat_start, flat_frag_stop_idx=flat_stop, mz=out_mz[:k], intensity=out_int[:k],
                   routes=dict(zip(("card_wave", "card_block", "select_wave", "select_block"), (int(r) for r in routes))),
                   kernel_ms=float(ms.value), h2d_bytes=int(link[0]), d2h_bytes=int(link[1]))
        for j, name in enumerate(("type", "loss_type", "charge", "number", "position", "cardinality")):
            out[name] = out_bytes[j, :k]
        if stage:
            self._staged_library((out["mz"],), k, None)
        return out

    # -- scoring ---------------------------------------------------------
    def score_host(self, cands: _abi.Marshalled, cfg_jit, with_stats: bool = False,
                   reuse_buffers: bool = False) -> dict:
        """Host table in, host OutputPsmDF arrays out (chunked, pipelined H2D / kernels / D2H).

        ``reuse_buffers=True`` writes into this context's page-locked output buffers (full PCIe
        rate, no allocation): the returned arrays are then only valid until the next such call."""
        n = int(cands.struct.n)
        # the call copies every table back completely: no need to clear the host buffers first
        alloc = (lambda name, shape, dt: self.pinned.empty("out:" + name, shape, dt)) if reuse_buffers else None
        # production calls (reuse_buffers) fetch exactly the OutputPsmDF tables; the diagnostic columns
        # (matched-peak counts, library slots) stay in HBM unless asked for
        width = _abi.output_width(cands, int(cfg_jit.top_k_fragments))
        if self.comm_world > 1:
            # the all-gather needs ONE table layout on all ranks: the widest shard decides (a collective)
            width = int(round(self.all_reduce_max(float(width))))
        m_out, arrays = _abi.alloc_output(n, width,
                                          with_stats=with_stats, zero=False, alloc=alloc,
                                          with_slots=with_stats or not reuse_buffers)
        cfg = _abi.pack_config(cfg_jit)
        self.tables_serial += 1
        _check(
            lib.adh_score_candidates(self._h, cands.ref(), C.byref(cfg), m_out.ref()),
            "adh_score_candidates",
        )
        self.n_candidates = n
        return arrays

    def score_host_compact(self, cands: _abi.Marshalled, cfg_jit, slots_per_row: float | None = None,
                           buffers: dict | None = None) -> dict:
        """``adh_score_candidates_compact``: the valid candidates and the filled fragment slots, column by column, in
        arrays this call allocates (the caller owns them): ``row``, ``precursor_idx``, ``rank``, ``features`` as
        [46, n_rows] (every feature a contiguous row) and the ``fragment_*`` columns per filled slot with
        ``fragment_row`` = row of the slot's candidate in the candidate table.

        The arrays are allocated at a capacity - all candidates, ``slots_per_row`` filled slots per candidate (default:
        the width of the padded tables, which always suffices) - and returned as views of their first n entries: the
        pages behind the unused tail of a large fresh allocation are never touched, so they cost address space only.
        A call whose ``slots_per_row`` turns out too small is repeated with what it needs.

        ``buffers``: a dict a caller keeps between calls of the same shape; the capacity arrays of the first call are
        parked in it and written again by the next ones (a steady-state loop - a benchmark, a search that scores batch
        after batch - then touches no fresh pages; the returned views are overwritten by the next call)."""
        n = int(cands.struct.n)
        width = _abi.output_width(cands, int(cfg_jit.top_k_fragments))
        cfg = _abi.pack_config(cfg_jit)
        rows_cap = max(n, 1)
        slots_cap = max(int(n * (width if slots_per_row is None else min(float(slots_per_row), width))) + 1, 1)
        self.tables_serial += 1
        while True:
            out = _abi.CompactOutput()
            out.rows_capacity, out.slots_capacity, out.top_k = rows_cap, slots_cap, width
            key = (rows_cap, slots_cap)
            arrays = buffers.get(key) if buffers is not None else None
            if arrays is None:
                arrays = {}
                for name, dt in _abi.COMPACT_ROW_FIELDS:
                    arrays[name] = np.empty(rows_cap, dtype=dt)
                arrays["features"] = np.empty((_abi.NUM_FEATURES, rows_cap), dtype=np.float32)
                for name, dt in _abi.COMPACT_SLOT_FIELDS:
                    arrays[name] = np.empty(slots_cap, dtype=dt)
                if buffers is not None:
                    buffers.clear()
                    buffers[key] = arrays
            for name, a in arrays.items():
                setattr(out, name, a.ctypes.data_as(dict(out._fields_)[name]))
            rc = lib.adh_score_candidates_compact(self._h, cands.ref(), C.byref(cfg), C.byref(out))
            if rc != 0 and (int(out.n_rows) > rows_cap or int(out.n_slots) > slots_cap):
                rows_cap, slots_cap = max(rows_cap, int(out.n_rows)), max(slots_cap, int(out.n_slots))
                continue  # (only a caller's own slots_per_row can be too small)
            _check(rc, "adh_score_candidates_compact")
            break
        self.n_candidates = n
        nr, ns = int(out.n_rows), int(out.n_slots)
        res = {name: arrays[name][:nr] for name, _ in _abi.COMPACT_ROW_FIELDS}
        res["features"] = arrays["features"][:, :nr]
        res.update({name: arrays[name][:ns] for name, _ in _abi.COMPACT_SLOT_FIELDS})
        res["top_k"] = width
        return res

    def score_resident(self, cands: _abi.Marshalled, cfg_jit) -> int:
        """``adh_score_candidates_resident``: score into this context's device tables and copy nothing back.  The
        tables (``device_tables``, ``fdr_resident``, ``take_rows``) are those ``score_host`` leaves; returns their width
        (fragment slots per row).  Refused while a communicator is attached."""
        n = int(cands.struct.n)
        cfg = _abi.pack_config(cfg_jit)
        self.tables_serial += 1
        _check(lib.adh_score_candidates_resident(self._h, cands.ref(), C.byref(cfg)), "adh_score_candidates_resident")
        self.n_candidates = n
        return _abi.output_width(cands, int(cfg_jit.top_k_fragments))

    def score_resident_append(self, cands: _abi.Marshalled, cfg_jit) -> tuple[int, int]:
        """``adh_score_candidates_resident_append``: score behind the rows accumulated since the last
        ``resident_reset`` (or the last other scoring call).  Returns ``(first_row, width)``: the table row of the
        batch's first candidate and the width of the accumulated tables."""
        cfg = _abi.pack_config(cfg_jit)
        first = C.c_int64(0)
        self.tables_serial += 1
        _check(lib.adh_score_candidates_resident_append(self._h, cands.ref(), C.byref(cfg), C.byref(first)),
               "adh_score_candidates_resident_append")
        self.n_candidates = int(cands.struct.n)
        return int(first.value), int(self.device_tables().top_k)

    def resident_reset(self) -> None:
        """``adh_resident_reset``: the device tables are empty; the next append starts at row 0."""
        self.tables_serial += 1
        _check(lib.adh_resident_reset(self._h), "adh_resident_reset")

    def resident_counts(self) -> tuple[int, int]:
        """``adh_resident_counts``: (valid rows, their filled fragment slots) of the current device tables."""
        rows, slots = C.c_int64(0), C.c_int64(0)
        _check(lib.adh_resident_counts(self._h, C.byref(rows), C.byref(slots)), "adh_resident_counts")
        return int(rows.value), int(slots.value)

    def take_rows(self, rows) -> dict:
        """``adh_take_rows``: the valid rows among the table rows ``rows`` of the current device tables, in list order,
        and their filled fragment slots - a dict with the keys and shapes of ``score_host_compact`` (``row`` and
        ``fragment_row`` are table rows).  Only these rows cross PCIe."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if r.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        width = int(self.device_tables().top_k)
        n = r.shape[0]
        rows_cap, slots_cap = max(n, 1), max(n * width, 1)
        while True:
            out = _abi.CompactOutput()
            out.rows_capacity, out.slots_capacity, out.top_k = rows_cap, slots_cap, width
            arrays = {name: np.empty(rows_cap, dtype=dt) for name, dt in _abi.COMPACT_ROW_FIELDS}
            arrays["features"] = np.empty((_abi.NUM_FEATURES, rows_cap), dtype=np.float32)
            arrays.update({name: np.empty(slots_cap, dtype=dt) for name, dt in _abi.COMPACT_SLOT_FIELDS})
            for name, a in arrays.items():
                setattr(out, name, a.ctypes.data_as(dict(out._fields_)[name]))
            rc = lib.adh_take_rows(self._h, _p(r, C.c_int64), n, C.byref(out))
            if rc != 0 and (int(out.n_rows) > rows_cap or int(out.n_slots) > slots_cap):
                rows_cap, slots_cap = max(rows_cap, int(out.n_rows)), max(slots_cap, int(out.n_slots))
                continue  # (cannot happen: every listed row and slot fits)
            _check(rc, "adh_take_rows")
            break
        nr, ns = int(out.n_rows), int(out.n_slots)
        res = {name: arrays[name][:nr] for name, _ in _abi.COMPACT_ROW_FIELDS}
        res["features"] = arrays["features"][:, :nr]
        res.update({name: arrays[name][:ns] for name, _ in _abi.COMPACT_SLOT_FIELDS})
        res["top_k"] = width
        return res

    def upload_candidates(self, cands: _abi.Marshalled) -> None:
        _check(lib.adh_upload_candidates(self._h, cands.ref()), "adh_upload_candidates")
        self.n_candidates = int(cands.struct.n)

    def stream_handle(self) -> int:
        """The context's own hipStream_t as an integer."""
        p = C.c_void_p()
        _check(lib.adh_get_stream(self._h, C.byref(p)), "adh_get_stream")
        return p.value or 0

    def score_uploaded(self, cfg_jit, out_struct: _abi.Output, stream: int = 0) -> None:
        """Enqueue scoring of the uploaded table into device buffers on ``stream`` (a raw
        hipStream_t; 0 = HIP's default stream); does not synchronise.  The caller must have
        zeroed the buffers on the same stream."""
        cfg = _abi.pack_config(cfg_jit)
        _check(
            lib.adh_score_uploaded(self._h, C.byref(cfg), C.byref(out_struct), stream),
            "adh_score_uploaded",
        )

    def synchronize(self) -> None:
        _check(lib.adh_synchronize(self._h), "adh_synchronize")

    def kernel_time_ms(self, reset: bool = True):
        """(gather_ms, feature_ms, launches): HIP-event averages per scoring call."""
        g = C.c_double(0)
        f = C.c_double(0)
        n = C.c_int64(0)
        _check(
            lib.adh_kernel_time_ms(self._h, C.byref(g), C.byref(f), C.byref(n), int(reset)),
            "adh_kernel_time_ms",
        )
        return g.value, f.value, n.value

    def plan_class_counts(self, reset: bool = False) -> np.ndarray:
        """Candidates per kernel class (the table in include/alphadia_hip.h) of every plan launched on this handle
        since the last reset, over all chunks and scoring entry points."""
        counts = np.zeros(_abi.N_PLAN_CLASSES, dtype=np.int64)
        _check(
            lib.adh_plan_class_counts(self._h, _p(counts, C.c_int64), int(reset)),
            "adh_plan_class_counts",
        )
        return counts

    def generic_launch_stats(self, reset: bool = False) -> dict:
        """Launch groups of the generic kernel class (small layouts, layouts up to the LDS of a CU, the spill path) of
        every plan launched on this handle since the last reset: ``candidates`` per group and the largest dynamic
        ``lds_bytes`` a launch of the group asked for."""
        stats = np.zeros(2 * _abi.N_GENERIC_GROUPS, dtype=np.int64)
        _check(
            lib.adh_generic_launch_stats(self._h, _p(stats, C.c_int64), int(reset)),
            "adh_generic_launch_stats",
        )
        return {"candidates": stats[: _abi.N_GENERIC_GROUPS].copy(), "lds_bytes": stats[_abi.N_GENERIC_GROUPS :].copy()}

    def im_launch_stats(self, reset: bool = False) -> dict:
        """Launch groups of the dynamic route of the ion-mobility feature kernel (small layouts, layouts up to the LDS of
        a CU, the spill path) of every plan launched on this handle since the last reset: ``candidates`` per group and
        the largest dynamic ``lds_bytes`` a launch of the group asked for."""
        stats = np.zeros(2 * _abi.N_IM_GROUPS, dtype=np.int64)
        _check(
            lib.adh_im_launch_stats(self._h, _p(stats, C.c_int64), int(reset)),
            "adh_im_launch_stats",
        )
        return {"candidates": stats[: _abi.N_IM_GROUPS].copy(), "lds_bytes": stats[_abi.N_IM_GROUPS :].copy()}

    # -- fragment competition -------------------------------------------
    def select_candidates(self, precursors: _abi.Marshalled, cfg, kernel) -> dict:
        """Candidate selection on the staged AlphaRaw run and library: packed precursor table in,
        the CandidateContainer arrays out (rows without a candidate keep score 0)."""
        c = _abi.pack_selection_config(cfg)
        k = np.ascontiguousarray(kernel, dtype=np.float32)
        if k.ndim != 2:
            raise ValueError("kernel must be 2-D (scan, cycle)")
        n = int(precursors.struct.n) * int(c.candidate_count)
        m_out, arrays = _abi.alloc_candidate_table(n)
        self.select_serial += 1
        _check(
            lib.adh_select_candidates(
                self._h, precursors.ref(), C.byref(c), _p(k, C.c_float), k.shape[0], k.shape[1], m_out.ref(),
            ),
            "adh_select_candidates",
        )
        return arrays

    # -- selection -> scoring hand-over in HBM ----------------------------
    def select_resident(self, precursors: _abi.Marshalled, cfg, kernel, elution_group_idx, decoy, channel) -> int:
        """``adh_select_candidates_resident``: the selection of ``select_candidates``, its table left in HBM with the
        precursor columns and the three id columns (one entry per precursor).  Returns the rows of the table."""
        c = _abi.pack_selection_config(cfg)
        k = np.ascontiguousarray(kernel, dtype=np.float32)
        if k.ndim != 2:
            raise ValueError("kernel must be 2-D (scan, cycle)")
        n = int(precursors.struct.n)
        eg, dc, ch = _abi.as_c(elution_group_idx, np.uint32), _abi.as_c(decoy, np.uint8), _abi.as_c(channel, np.uint8)
        if eg.shape != (n,) or dc.shape != (n,) or ch.shape != (n,):
            raise ValueError("elution_group_idx / decoy / channel must hold one entry per precursor")
        self.select_serial += 1
        _check(
            lib.adh_select_candidates_resident(
                self._h, precursors.ref(), C.byref(c), _p(k, C.c_float), k.shape[0], k.shape[1], _p(eg, C.c_uint32),
                _p(dc, C.c_uint8), _p(ch, C.c_uint8)),
            "adh_select_candidates_resident",
        )
        return n * int(c.candidate_count)

    def assemble_selected(self, apply_cutoff: bool, score_cutoff: float, score_grouped: bool,
                          reference_channel: int) -> tuple[int, int, bool]:
        """``adh_assemble_selected`` on the table of ``select_resident``: ``(n_selected, n_kept, was_sorted)``.  The
        cutoff is rounded to the dtype NumPy compares a float32 column with it in (the device compares in float64)."""
        cutoff = float(np.asarray(score_cutoff).astype(np.result_type(np.float32, score_cutoff)))
        n_sel, n_kept, was_sorted = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(lib.adh_assemble_selected(self._h, int(bool(apply_cutoff)), cutoff, int(bool(score_grouped)),
                                         int(reference_channel), C.byref(n_sel), C.byref(n_kept), C.byref(was_sorted)),
               "adh_assemble_selected")
        return int(n_sel.value), int(n_kept.value), bool(was_sorted.value)

    def select_handover_stats(self) -> dict:
        """``adh_select_handover_stats``: what the last ``assemble_selected`` did."""
        stats, ms = (C.c_int32 * 4)(), C.c_double(0.0)
        _check(lib.adh_select_handover_stats(self._h, stats, C.byref(ms)), "adh_select_handover_stats")
        return {"was_sorted": bool(stats[0]), "radix_passes": int(stats[1]), "group_scans": int(stats[2]),
                "skipped_rows": int(stats[3]), "assemble_ms": float(ms.value)}

    def score_selected_resident(self, cfg_jit) -> int:
        """``adh_score_selected_resident``: ``score_resident`` on the table ``assemble_selected`` left in HBM; returns
        the width of the device tables."""
        cfg = _abi.pack_config(cfg_jit)
        self.tables_serial += 1
        _check(lib.adh_score_selected_resident(self._h, C.byref(cfg)), "adh_score_selected_resident")
        view = self.device_tables()
        self.n_candidates = int(view.n)
        return int(view.top_k)

    def selected_ids(self, n: int) -> tuple[np.ndarray, np.ndarray]:
        """``adh_selected_ids``: (row in the selection table, rank) of the ``n`` rows of the assembled table."""
        rows, rank = np.empty(n, np.uint32), np.empty(n, np.uint8)
        _check(lib.adh_selected_ids(self._h, _p(rows, C.c_uint32), _p(rank, C.c_uint8), n), "adh_selected_ids")
        return rows, rank

    def take_selected(self, rows) -> tuple[dict, np.ndarray]:
        """``adh_take_selected``: the nine candidate columns of the listed rows of the assembled table, and their
        positions among the rows with score > 0."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if r.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        m_out, arrays = _abi.alloc_candidate_table(r.shape[0])
        pos = np.zeros(r.shape[0], np.uint32)
        _check(lib.adh_take_selected(self._h, _p(r, C.c_int64), r.shape[0], m_out.ref(),
                                     _p(pos, C.c_uint32)), "adh_take_selected")
        return arrays, pos

    def select_time_ms(self) -> float:
        ms = C.c_double(0.0)
        _check(lib.adh_select_time_ms(self._h, C.byref(ms)), "adh_select_time_ms")
        return float(ms.value)

    def transpose_timstof(self, tof_indices, push_indptr, n_tof_indices: int, values):
        """Drop-in for ``_transpose`` (alphadia/raw_data/bruker.py:201-280): returns
        ``(push_indices, tof_indptr, new_values)`` in the TOF-major layout."""
        tof = _abi.as_c(tof_indices, np.uint32)
        ptr = _abi.as_c(push_indptr, np.int64)
        val = np.ascontiguousarray(values, dtype=np.uint16)
        n = tof.shape[0]
        if val.shape[0] != n or ptr.shape[0] < 1:
            raise ValueError("tof_indices / values / push_indptr have inconsistent lengths")
        push_out = np.zeros(n, dtype=np.uint32)
        val_out = np.zeros(n, dtype=np.uint16)
        indptr_out = np.zeros(int(n_tof_indices) + 1, dtype=np.int64)
        _check(
            lib.adh_transpose_timstof(
                self._h, _p(tof, C.c_uint32), _p(ptr, C.c_int64), ptr.shape[0] - 1, int(n_tof_indices), _p(val, C.c_uint16),
                n, _p(push_out, C.c_uint32), _p(indptr_out, C.c_int64), _p(val_out, C.c_uint16),
            ),
            "adh_transpose_timstof",
        )
        return push_out, indptr_out, val_out

    def fragcomp(self, window_start, window_stop, rt, frag_start, frag_stop, fragment_mz,
                 rt_tol_seconds: float, mass_tol_ppm: float, valid=None) -> np.ndarray:
        ws = _abi.as_c(window_start, np.int64)
        we = _abi.as_c(window_stop, np.int64)
        rtv = _abi.as_c(rt, np.float32)
        fs = _abi.as_c(frag_start, np.int64)
        fe = _abi.as_c(frag_stop, np.int64)
        fm = _abi.as_c(fragment_mz, np.float32)
        # the reference starts from an all-true column (fragcomp.py:281); `valid` lets a caller start from less
        valid = (np.ones(rtv.shape[0], dtype=np.uint8) if valid is None
                 else np.array(valid, dtype=bool).astype(np.uint8))
        if valid.shape[0] != rtv.shape[0] or fs.shape[0] != rtv.shape[0] or fe.shape[0] != rtv.shape[0]:
            raise ValueError("rt / fragment ranges / valid must have one entry per PSM")
        _check(
            lib.adh_fragcomp(
                self._h, ws.shape[0], _p(ws, C.c_int64), _p(we, C.c_int64), rtv.shape[0], _p(rtv, C.c_float),
                _p(fs, C.c_int64), _p(fe, C.c_int64), fm.shape[0], _p(fm, C.c_float), rt_tol_seconds, mass_tol_ppm,
                _p(valid, C.c_uint8),
            ),
            "adh_fragcomp",
        )
        return valid.view(np.bool_)

    def fragcomp_frames(self, psm_precursor_idx, psm_rank, psm_mz_observed, psm_rt_observed, psm_proba,
                        frag_precursor_idx, frag_rank, frag_mz_observed, cycle, rt_tol_seconds: float, mass_tol_ppm: float):
        """``adh_fragcomp_frames``: plan and competition on the device from the frames' columns.  Returns
        ``(rows, valid)`` - input position and flag of every processed PSM in processing order - or ``None`` when the
        fragment table is not grouped by candidate (the caller prepares the plan itself)."""
        pp, pr = _abi.as_c(psm_precursor_idx, np.uint32), _abi.as_c(psm_rank, np.uint8)
        pmz, prt = _abi.as_c(psm_mz_observed, np.float32), _abi.as_c(psm_rt_observed, np.float32)
        ppb = _abi.as_c(psm_proba, np.float32)
        fp, fr = _abi.as_c(frag_precursor_idx, np.uint32), _abi.as_c(frag_rank, np.uint8)
        fmz = _abi.as_c(frag_mz_observed, np.float32)
        lower = np.ascontiguousarray(cycle[0, :, :, 0].min(axis=1), dtype=np.float64)
        upper = np.ascontiguousarray(cycle[0, :, :, 1].max(axis=1), dtype=np.float64)
        n = pp.shape[0]
        if not (pr.shape[0] == pmz.shape[0] == prt.shape[0] == ppb.shape[0] == n) or fr.shape[0] != fp.shape[0] \
                or fmz.shape[0] != fp.shape[0]:
            raise ValueError("columns of one frame differ in length")
        rows, valid = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.uint8)
        n_rows, grouped = C.c_int64(0), C.c_int32(1)
        _check(
            lib.adh_fragcomp_frames(
                self._h, n, _p(pp, C.c_uint32), _p(pr, C.c_uint8), _p(pmz, C.c_float), _p(prt, C.c_float),
                _p(ppb, C.c_float), fp.shape[0], _p(fp, C.c_uint32), _p(fr, C.c_uint8), _p(fmz, C.c_float),
                lower.shape[0], _p(lower, C.c_double), _p(upper, C.c_double), rt_tol_seconds, mass_tol_ppm,
                _p(rows, C.c_int64), _p(valid, C.c_uint8), C.byref(n_rows), C.byref(grouped)),
            "adh_fragcomp_frames",
        )
        if not grouped.value:
            return None
        k = int(n_rows.value)
        return rows[:k], valid[:k].astype(bool)

    def fragcomp_stats(self) -> dict:
        """``adh_fragcomp_stats``: device time and work counters of the last competition."""
        ms = C.c_double(0.0)
        pairs, waiting = C.c_int64(0), C.c_int64(0)
        rounds, serial = C.c_int32(0), C.c_int32(0)
        _check(lib.adh_fragcomp_stats(self._h, C.byref(ms), C.byref(pairs), C.byref(waiting), C.byref(rounds),
                                      C.byref(serial)), "adh_fragcomp_stats")
        return dict(kernel_ms=ms.value, pairs=pairs.value, waiting=waiting.value, rounds=rounds.value,
                    serial=bool(serial.value))


    # -- FDR stage ---------------------------------------------------------
    def fdr_q_values(self, score, decoy, tiebreak=None):
        """``get_q_values`` (alphadia/fdr/fdr.py:232-297): returns ``(order, qval)``, the input row
        at every sorted position and its q-value."""
        sc = _abi.as_c(score, np.float64)
        de = _abi.as_c(np.asarray(decoy) != 0, np.uint8)
        n = sc.shape[0]
        if de.shape[0] != n:
            raise ValueError("score and decoy differ in length")
        tb = None
        if tiebreak is not None:
            tb = _abi.as_c(tiebreak, np.int64)
            if tb.shape[0] != n:
                raise ValueError("score and tiebreak differ in length")
        order = np.zeros(n, dtype=np.int64)
        qval = np.zeros(n, dtype=np.float64)
        _check(
            lib.adh_fdr_q_values(self._h, n, _p(sc, C.c_double), _p(de, C.c_uint8), _p(tb, C.c_int64), _p(order, C.c_int64),
                                 _p(qval, C.c_double)),
            "adh_fdr_q_values",
        )
        return order, qval

    def fdr_keep_best(self, score, group_a, group_b=None) -> np.ndarray:
        """``keep_best`` (alphadia/fdr/fdr.py:181-213) as a mask over the input rows."""
        sc = _abi.as_c(score, np.float64)
        ga = _abi.as_c(group_a, np.int64)
        gb = _abi.as_c(group_b, np.int64) if group_b is not None else None
        n = sc.shape[0]
        if ga.shape[0] != n or (gb is not None and gb.shape[0] != n):
            raise ValueError("score and group columns differ in length")
        keep = np.zeros(n, dtype=np.uint8)
        _check(
            lib.adh_fdr_keep_best(self._h, n, _p(sc, C.c_double), _p(ga, C.c_int64), _p(gb, C.c_int64), _p(keep, C.c_uint8)),
            "adh_fdr_keep_best",
        )
        return keep.view(np.bool_)

    # -- library calibration ---------------------------------------------
    def calibration_predict(self, model, x) -> np.ndarray:
        """``adh_calibration_predict``: ``LOESSRegression.predict`` (alphadia/calibration/models.py:276-300) of a
        fitted model - anything with ``scale_mean``, ``scale_max`` and ``beta[d, k]`` - over a float32 or float64
        column, host -> host.  Other dtypes are taken as float64.  Returns float64."""
        packed = _abi.pack_loess_model(model.scale_mean, model.scale_max, model.beta)
        xa = np.asarray(x)
        if xa.ndim == 2 and xa.shape[1] == 1:
            xa = xa[:, 0]
        if xa.ndim != 1:
            raise ValueError("calibration_predict takes one input column")
        xa = np.ascontiguousarray(xa, dtype=np.float32 if xa.dtype == np.float32 else np.float64)
        y = np.empty(xa.shape[0], dtype=np.float64)
        _check(lib.adh_calibration_predict(self._h, C.byref(packed), _p(xa), int(xa.dtype == np.float64), xa.shape[0],
                                           _p(y, C.c_double)), "adh_calibration_predict")
        return y

    def calibration_time_ms(self) -> float:
        """HIP-event time of the kernels of the last ``calibration_predict`` call."""
        ms = C.c_double(0.0)
        _check(lib.adh_calibration_time_ms(self._h, C.byref(ms)), "adh_calibration_time_ms")
        return float(ms.value)

    # -- fragment quantity matrices (label-free quantification) -----------
    def quant_matrices(self, n_columns: int, psm_precursor_idx) -> DeviceQuant:
        """An empty ``adh_quant_t``: the cross-run quantity matrices of ``n_columns`` float32 columns over the frag
        rows whose precursor is in ``psm_precursor_idx``."""
        return DeviceQuant(self, n_columns, psm_precursor_idx)

    # -- protein inference ------------------------------------------------
    def protein_groups(self) -> DeviceProteinGroups:
        """An ``adh_pg_t``: the greedy set cover of protein inference, one cover per connected component."""
        return DeviceProteinGroups(self)

    # -- protein-group FDR ------------------------------------------------
    def protein_fdr(self) -> DeviceProteinFdr:
        """An ``adh_pfdr_t``: group features, the classifier and the gather of the protein-group FDR."""
        return DeviceProteinFdr(self)

    # -- transfer-learning library ----------------------------------------
    def transfer_library(self, n_columns: int, n_matrices: int) -> DeviceTransferLibrary:
        """An empty ``adh_tl_t``: the consensus of the transfer-learning accumulator, ``n_matrices`` dense float32
        matrices of ``n_columns`` columns."""
        return DeviceTransferLibrary(self, n_columns, n_matrices)

    def tl_qc(self, frag_start, frag_stop, intensity, correlation, cutoff, ratio, empty_passes: bool):
        """``adh_tl_qc``: ``(use_for_ms2, masked intensity, blocks on the workgroup path, kernel ms)``; ``intensity``
        is not modified."""
        fs, fe = _abi.as_c(frag_start, np.int64), _abi.as_c(frag_stop, np.int64)
        inten = np.array(intensity, dtype=np.float32, order="C", ndmin=2)
        corr = _abi.as_c(correlation, np.float32)
        if corr.shape != inten.shape or fs.ndim != 1 or fe.shape != fs.shape:
            raise ValueError("tl_qc: intensity and correlation of one shape, one start and stop per precursor")
        use = np.zeros(fs.shape[0], np.uint8)
        large, ms = C.c_int64(0), C.c_double(0.0)
        _check(lib.adh_tl_qc(self._h, fs.shape[0], _p(fs, C.c_int64), _p(fe, C.c_int64), inten.shape[0], inten.shape[1],
                             _p(inten, C.c_float), _p(corr, C.c_float), cutoff, ratio, int(bool(empty_passes)),
                             _p(use, C.c_uint8), C.byref(large), C.byref(ms)), "adh_tl_qc")
        return use.astype(bool), inten, int(large.value), float(ms.value)

    def tl_rt_norm(self, rt_observed, rt_calibrated=None, rt_library=None):
        """``adh_tl_rt_norm``: ``(rt_norm, kernel ms)``; max normalisation when ``rt_calibrated`` is None."""
        def col(a):
            a = np.asarray(a)
            return np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)

        obs = col(rt_observed)
        delta = rt_calibrated is not None
        cal, lb = (col(rt_calibrated), col(rt_library)) if delta else (None, None)
        if obs.ndim != 1 or (delta and (cal.shape != obs.shape or lb.shape != obs.shape)):
            raise ValueError("tl_rt_norm: one value of every column per row")
        out = np.empty(obs.shape[0], np.result_type(obs, cal, lb) if delta else obs.dtype)
        ms = C.c_double(0.0)
        f64 = lambda a: int(a is not None and a.dtype == np.float64)  # noqa: E731
        _check(lib.adh_tl_rt_norm(self._h, obs.shape[0], int(delta), _p(obs), f64(obs), _p(cal), f64(cal), _p(lb),
                                  f64(lb), _p(out), C.byref(ms)), "adh_tl_rt_norm")
        return out, float(ms.value)

    # -- match-between-runs library ---------------------------------------
    def mbr_library(self) -> DeviceMbr:
        """An ``adh_mbr_t``: the aggregate tables, the passed elution groups and the filtered library in HBM."""
        return DeviceMbr(self)


class _DeviceSession:
    """A native object that lives on a ``Context``'s handle (``adh_mlp_t``, ``adh_quant_t``, ...).  The subclass
    fills ``self._s`` with its create call.  The context closes its live sessions before it destroys the handle, so
    the native destroy always finds the handle it reads, and a session closed that way makes no native call later.
    (The subclass makes its own destroy and ``time_ms`` calls by name, as every native call in this module is spelled
    ``lib.adh_<name>(...)``: the ABI tests read the module and the wrapper classes for the exports they call.)"""

    def __init__(self, ctx: Context):
        self._ctx = ctx  # keeps the handle alive
        self._s = C.c_void_p()
        ctx._sessions.add(self)

    def _native_destroy(self, s):
        """The subclass calls its destroy export on ``s``."""
        raise NotImplementedError

    def close(self):
        s = getattr(self, "_s", None)  # (absent when __init__ failed early)
        if s:
            self._s = C.c_void_p()
            self._native_destroy(s)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _times(n: int, call) -> tuple:
        """The ``n`` HIP-event times (ms) that ``call`` fills: it gets ``n`` doubles by reference and returns the
        status of a ``*_time_ms`` export."""
        t = [C.c_double(0.0) for _ in range(n)]
        _check(call(*(C.byref(x) for x in t)), "time_ms")
        return tuple(float(x.value) for x in t)


class DeviceMlp(_DeviceSession):
    """An ``adh_mlp_t``: the classifier network with its parameters, optimiser moments and the
    staged feature matrix in HBM."""

    def __init__(self, ctx: Context, input_dim: int, layers, output_dim: int = 2):
        super().__init__(ctx)
        self.arch = _abi.pack_mlp_arch(input_dim, layers, output_dim)
        self.input_dim, self.layers, self.output_dim = int(input_dim), [int(x) for x in layers], int(output_dim)
        n = C.c_int64(0)
        _check(lib.adh_mlp_param_count(C.byref(self.arch), C.byref(n)), "adh_mlp_param_count")
        self.n_params = int(n.value)
        _check(lib.adh_mlp_create(ctx._h, C.byref(self.arch), C.byref(self._s)), "adh_mlp_create")
        self.n_rows = 0

    def _native_destroy(self, s):
        lib.adh_mlp_destroy(s)

    def set_state(self, params, running_mean, running_var, num_batches_tracked: int = 0):
        pa = _abi.as_c(params, np.float32)
        rm = _abi.as_c(running_mean, np.float32)
        rv = _abi.as_c(running_var, np.float32)
        if pa.shape != (self.n_params,) or rm.shape != (self.input_dim,) or rv.shape != (self.input_dim,):
            raise ValueError("state arrays do not match the architecture")
        _check(lib.adh_mlp_set_state(self._s, _p(pa, C.c_float), _p(rm, C.c_float), _p(rv, C.c_float),
                                     int(num_batches_tracked)), "adh_mlp_set_state")

    def get_state(self):
        pa = np.zeros(self.n_params, dtype=np.float32)
        rm = np.zeros(self.input_dim, dtype=np.float32)
        rv = np.zeros(self.input_dim, dtype=np.float32)
        nbt = C.c_int64(0)
        _check(lib.adh_mlp_get_state(self._s, _p(pa, C.c_float), _p(rm, C.c_float), _p(rv, C.c_float),
                                     C.byref(nbt)), "adh_mlp_get_state")
        return pa, rm, rv, int(nbt.value)

    def stage_rows(self, x, y=None):
        xa = _abi.as_c(x, np.float32)
        if xa.ndim != 2:
            raise ValueError("x must be (n_samples, n_features)")
        ya = None
        if y is not None:
            ya = _abi.as_c(y, np.float32)
            if ya.shape != (xa.shape[0],):
                raise ValueError("y must hold one target per row")
        _check(lib.adh_mlp_stage_rows(self._s, _p(xa, C.c_float), xa.shape[0], xa.shape[1], _p(ya, C.c_float)),
               "adh_mlp_stage_rows")
        self.n_rows = xa.shape[0]

    def stage_rows_device(self, src_cols, decoy, extra_cols=(), channel=None, part=None):
        """Stage the usable rows of the device tables of the last ``score_host`` call (targets first,
        then decoys); returns ``(n_targets, n_decoys)``.  See ``adh_mlp_stage_rows_device``.

        ``part = (target_channel, decoy_channel, label_by_channel)`` stages one part of a channel-wise decoy
        strategy instead (``adh_mlp_stage_rows_device_part``): the rows whose ``channel`` is the target or the decoy
        channel (-1: none), labelled by the decoy channel if ``label_by_channel`` and by ``decoy`` otherwise."""
        sc = _abi.as_c(src_cols, np.int32)
        de = _abi.as_c(np.asarray(decoy) != 0, np.uint8)
        extras = [_abi.as_c(e, np.float32) for e in extra_cols]
        if any(e.shape != de.shape for e in extras):
            raise ValueError("extra columns must have one value per candidate row")
        arr = (C.POINTER(C.c_float) * max(len(extras), 1))(*[_p(e, C.c_float) for e in extras])
        nt, nd = C.c_int64(0), C.c_int64(0)
        if part is None:
            _check(lib.adh_mlp_stage_rows_device(self._s, _p(sc, C.c_int32), sc.shape[0], arr, len(extras), _p(de, C.c_uint8),
                                                 de.shape[0], C.byref(nt), C.byref(nd)), "adh_mlp_stage_rows_device")
        else:
            if channel is None:
                raise ValueError("a part needs the channel column")
            ch = _abi.as_c(channel, np.int64)
            if ch.shape != de.shape:
                raise HipBackendError(f"channel holds {ch.shape[0] if ch.ndim == 1 else ch.shape} values, decoy "
                                      f"{de.shape[0]}: one per row of the device tables is needed")
            target, decoy_channel, by_channel = part
            _check(lib.adh_mlp_stage_rows_device_part(
                self._s, _p(sc, C.c_int32), sc.shape[0], arr, len(extras), _p(de, C.c_uint8), de.shape[0], _p(ch, C.c_int64),
                int(target), int(decoy_channel), int(bool(by_channel)), C.byref(nt), C.byref(nd)),
                "adh_mlp_stage_rows_device_part")
        self.n_rows = int(nt.value) + int(nd.value)
        return int(nt.value), int(nd.value)

    def staged_rows(self) -> np.ndarray:
        rows = np.zeros(self.n_rows, dtype=np.int64)
        _check(lib.adh_mlp_staged_rows(self._s, _p(rows, C.c_int64), rows.shape[0]), "adh_mlp_staged_rows")
        return rows

    def predict_resident(self) -> None:
        _check(lib.adh_mlp_predict_resident(self._s), "adh_mlp_predict_resident")

    def fit(self, train_rows, batch_start, batch_size: int, learning_rate: float, weight_decay: float,
            dropout: float, seed: int = 0, first_step: int = 0, betas=(0.9, 0.999), eps: float = 1e-8) -> np.ndarray:
        tr = _abi.as_c(train_rows, np.int64)
        bs = _abi.as_c(batch_start, np.int64)
        f = _abi.MlpFit()
        f.train_rows, f.n_train = _p(tr, C.c_int64), tr.shape[0]
        f.batch_start, f.n_steps = _p(bs, C.c_int64), bs.shape[0]
        f.batch_size = int(batch_size)
        f.learning_rate, f.weight_decay, f.dropout = float(learning_rate), float(weight_decay), float(dropout)
        f.beta1, f.beta2, f.eps = float(betas[0]), float(betas[1]), float(eps)
        f.seed, f.first_step = int(seed) & (2**64 - 1), int(first_step)
        loss = np.zeros(bs.shape[0], dtype=np.float32)
        _check(lib.adh_mlp_fit(self._s, C.byref(f), _p(loss, C.c_float)), "adh_mlp_fit")
        return loss

    def predict(self, rows=None) -> np.ndarray:
        if rows is None:
            n, rp = self.n_rows, None
        else:
            ra = _abi.as_c(rows, np.int64)
            n, rp = ra.shape[0], _p(ra, C.c_int64)
        out = np.zeros((n, self.output_dim), dtype=np.float32)
        _check(lib.adh_mlp_predict(self._s, rp, n, _p(out, C.c_float)), "adh_mlp_predict")
        return out

    def time_ms(self):
        return self._times(2, lambda *t: lib.adh_mlp_time_ms(self._s, *t))


class DeviceQuant(_DeviceSession):
    """An ``adh_quant_t``: the kept frag rows of every run, then their union of ion keys and one column-major
    ``n_keys x n_runs`` float32 matrix per quantity column, in HBM (include/alphadia_hip.h: adh_quant_*)."""

    def __init__(self, ctx: Context, n_columns: int, psm_precursor_idx):
        super().__init__(ctx)
        self.n_columns = int(n_columns)
        psm = np.ascontiguousarray(psm_precursor_idx, dtype=np.uint32)
        _check(lib.adh_quant_create(ctx._h, self.n_columns, _p(psm, C.c_uint32), psm.shape[0],
                                    C.byref(self._s)), "adh_quant_create")
        self.n_runs = 0
        self.n_rows = 0
        self.n_keys = 0
        self.duplicate = False

    def _native_destroy(self, s):
        lib.adh_quant_destroy(s)

    @staticmethod
    def _cols(arrays):
        return (C.POINTER(C.c_float) * max(len(arrays), 1))(*[_p(a, C.c_float) for a in arrays])

    def add_run(self, precursor_idx, number, type_, charge, loss_type, columns) -> int:
        """Append one run (uint32 precursor_idx, four uint8 columns, ``n_columns`` float32 columns); returns the rows
        kept."""
        p = _abi.as_c(precursor_idx, np.uint32)
        b = [_abi.as_c(x, np.uint8) for x in (number, type_, charge, loss_type)]
        cols = [_abi.as_c(x, np.float32) for x in columns]
        n = p.shape[0]
        if len(cols) != self.n_columns or any(x.shape != (n,) for x in [*b, *cols]):
            raise ValueError("add_run: every column must hold one value per row, one array per quantity column")
        kept = C.c_int64(0)
        _check(lib.adh_quant_add_run(self._s, n, _p(p, C.c_uint32), *[_p(x, C.c_uint8) for x in b],
                                     self._cols(cols), C.byref(kept)), "adh_quant_add_run")
        self.n_runs += 1
        self.n_rows += int(kept.value)
        return int(kept.value)

    def build(self) -> tuple[int, bool]:
        """The union of keys and the matrices; returns ``(n_keys, duplicate)``."""
        nk, dup = C.c_int64(0), C.c_int32(0)
        _check(lib.adh_quant_build(self._s, C.byref(nk), C.byref(dup)), "adh_quant_build")
        self.n_keys, self.duplicate = int(nk.value), bool(dup.value)
        return self.n_keys, self.duplicate

    def keys(self):
        ion = np.empty(self.n_keys, dtype=np.int64)
        pidx = np.empty(self.n_keys, dtype=np.uint32)
        _check(lib.adh_quant_keys(self._s, _p(ion, C.c_int64), _p(pidx, C.c_uint32)), "adh_quant_keys")
        return ion, pidx

    def matrix(self, column: int) -> np.ndarray:
        """Quantity column ``column`` as a C-ordered ``(n_runs, n_keys)`` float32 array (one row per run)."""
        out = np.empty((self.n_runs, self.n_keys), dtype=np.float32)
        _check(lib.adh_quant_matrix(self._s, int(column), _p(out, C.c_float)), "adh_quant_matrix")
        return out

    def rows(self):
        """The appended rows in run order: ``(ion, precursor_idx, run, [columns])``."""
        n = self.n_rows
        ion, pidx, run = np.empty(n, np.int64), np.empty(n, np.uint32), np.empty(n, np.uint32)
        cols = [np.empty(n, np.float32) for _ in range(self.n_columns)]
        _check(lib.adh_quant_rows(self._s, _p(ion, C.c_int64), _p(pidx, C.c_uint32), _p(run, C.c_uint32), self._cols(cols)),
               "adh_quant_rows")
        return ion, pidx, run, cols

    def set_matrix(self, run_columns) -> None:
        """A fresh one-column object takes its quality matrix from the host: one float32 array per run."""
        cols = [_abi.as_c(x, np.float32) for x in run_columns]
        n = cols[0].shape[0] if cols else 0
        if any(c.shape != (n,) for c in cols):
            raise ValueError("set_matrix: run columns differ in length")
        _check(lib.adh_quant_set_matrix(self._s, n, len(cols), self._cols(cols)), "adh_quant_set_matrix")
        self.n_runs, self.n_keys = len(cols), n

    def filter(self, column: int, group, n_groups: int, top_n: float, threshold: float):
        """``(total, rank, mask)`` of ``adh_quant_filter`` over matrix ``column``."""
        g = _abi.as_c(group, np.int32)
        if g.shape != (self.n_keys,):
            raise ValueError("filter: one group code per key row")
        total = np.empty(self.n_keys, np.float32)
        rank = np.empty(self.n_keys, np.float64)
        mask = np.empty(self.n_keys, np.uint8)
        _check(lib.adh_quant_filter(self._s, int(column), _p(g, C.c_int32), int(n_groups), top_n, threshold,
                                    _p(total, C.c_float), _p(rank, C.c_double), _p(mask, C.c_uint8)), "adh_quant_filter")
        return total, rank, mask.view(np.bool_)

    def time_ms(self):
        """HIP-event times (ms) of the build and of the last filter."""
        return self._times(2, lambda *t: lib.adh_quant_time_ms(self._s, *t))

    def lfq(self, column: int, keep, group, n_groups: int, min_nonan: int, num_samples_quadratic: int,
            normalize: bool):
        """Label-free quantification over matrix ``column`` (include/alphadia_hip_lfq.h: adlfq_run): ``keep`` a mask
        over the key rows or None, ``group`` one code per key row.  Returns the kept group codes (ascending) and
        their ``(n_kept, n_runs)`` float64 table."""
        g = _abi.as_c(group, np.int32)
        k = None if keep is None else _abi.as_c(np.asarray(keep) != 0, np.uint8)
        if g.shape != (self.n_keys,) or (k is not None and k.shape != g.shape):
            raise ValueError("lfq: one group code (and one mask value) per key row")
        n = C.c_int64(0)
        _check(lib.adlfq_run(self._s, int(column), _p(k, C.c_uint8), _p(g, C.c_int32), int(n_groups), int(min_nonan),
                             int(num_samples_quadratic), int(bool(normalize)), C.byref(n)), "adlfq_run")
        groups = np.empty(n.value, dtype=np.int32)
        table = np.empty((n.value, self.n_runs), dtype=np.float64)
        _check(lib.adlfq_result(self._s, _p(groups, C.c_int32), _p(table, C.c_double)), "adlfq_result")
        return groups, table

    def lfq_time_ms(self):
        """HIP-event times (ms) of the last ``lfq``: prepare, sample normalisation, group kernels."""
        return self._times(3, lambda *t: lib.adlfq_time_ms(self._s, *t))


class DeviceProteinGroups(_DeviceSession):
    """An ``adh_pg_t``: the set cover of protein inference over (pattern, id) edges and its heuristic filter
    (include/alphadia_hip.h: adh_pg_*)."""

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        _check(lib.adh_pg_create(ctx._h, C.byref(self._s)), "adh_pg_create")
        self.n_patterns = self.n_ids = self.n_edges = 0

    def _native_destroy(self, s):
        lib.adh_pg_destroy(s)

    def solve(self, edge_pattern, edge_id, weight, n_ids: int):
        """``(pattern_master, id_emptied_by)`` of ``adh_pg_solve``: one weight per pattern, ``n_ids`` id codes."""
        ep, ei, w = (_abi.as_c(x, np.int32) for x in (edge_pattern, edge_id, weight))
        if ep.ndim != 1 or ep.shape != ei.shape or w.ndim != 1:
            raise ValueError("solve: one pattern and one id per edge, one weight per pattern")
        master = np.empty(w.shape[0], np.int32)
        emptied = np.empty(max(int(n_ids), 0), np.int32)
        _check(lib.adh_pg_solve(self._s, w.shape[0], int(n_ids), ep.shape[0], _p(ep, C.c_int32), _p(ei, C.c_int32),
                                _p(w, C.c_int32), _p(master, C.c_int32), _p(emptied, C.c_int32)), "adh_pg_solve")
        self.n_patterns, self.n_ids, self.n_edges = w.shape[0], int(n_ids), ep.shape[0]
        return master, emptied

    def filter(self, id_string, id_rank, n_strings: int):
        """``(offsets, ids)`` of ``adh_pg_filter``: per pattern, its ids whose string a master carries, by rank."""
        s, r = _abi.as_c(id_string, np.int32), _abi.as_c(id_rank, np.int32)
        if s.shape != (self.n_ids,) or r.shape != (self.n_ids,):
            raise ValueError("filter: one string code and one rank per id of the last solve")
        off = np.empty(self.n_patterns + 1, np.int32)
        ids = np.empty(max(self.n_edges, 1), np.int32)
        kept = C.c_int64(0)
        _check(lib.adh_pg_filter(self._s, int(n_strings), _p(s, C.c_int32), _p(r, C.c_int32), _p(off, C.c_int32),
                                 _p(ids, C.c_int32), C.byref(kept)), "adh_pg_filter")
        return off, ids[: int(kept.value)]

    def stats(self) -> tuple[int, int, int]:
        """(components, components of more than 64 ids, labelling rounds) of the last solve."""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(lib.adh_pg_stats(self._s, C.byref(a), C.byref(b), C.byref(c)), "adh_pg_stats")
        return int(a.value), int(b.value), int(c.value)

    def time_ms(self) -> tuple[float, float, float]:
        """HIP-event times (ms) of the component labelling, the cover and the filter."""
        return self._times(3, lambda *t: lib.adh_pg_time_ms(self._s, *t))


class DeviceProteinFdr(_DeviceSession):
    """An ``adh_pfdr_t``: the (pg, decoy) group features of a precursor table, sklearn's MLPClassifier trained one
    epoch per launch, and the gather of a per-group value to the rows (include/alphadia_hip.h: adh_pfdr_*)."""

    N_FEATURES = 7
    N_PARAMS = 901

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        _check(lib.adh_pfdr_create(ctx._h, C.byref(self._s)), "adh_pfdr_create")
        self.n_rows = self.n_groups = self.n_train = 0

    def _native_destroy(self, s):
        lib.adh_pfdr_destroy(s)

    def features(self, pg, decoy, precursor_idx, sequence, run, proba, with_row_group: bool = False):
        """``(group_pg, group_decoy, features [groups, 7])`` of ``adh_pfdr_features``, the groups ascending by
        (pg, decoy); with ``with_row_group`` also the group of every row (-1: none)."""
        pg, seq, rn = (_abi.as_c(x, np.int32) for x in (pg, sequence, run))
        de = _abi.as_c(decoy, np.uint8)
        pi = _abi.as_c(precursor_idx, np.int64)
        pr = np.asarray(proba)
        pr = np.ascontiguousarray(pr, dtype=np.float32 if pr.dtype == np.float32 else np.float64)
        n = pg.shape[0]
        if pg.ndim != 1 or any(a.shape != (n,) for a in (seq, rn, de, pi, pr)):
            raise ValueError("features: one value of every column per row")
        groups = C.c_int64(0)
        _check(lib.adh_pfdr_features(self._s, n, _p(pg, C.c_int32), _p(de, C.c_uint8), _p(pi, C.c_int64),
                                     _p(seq, C.c_int32), _p(rn, C.c_int32), _p(pr),
                                     int(pr.dtype == np.float64), C.byref(groups)), "adh_pfdr_features")
        self.n_rows, self.n_groups = n, int(groups.value)
        gpg = np.empty(self.n_groups, np.int32)
        gde = np.empty(self.n_groups, np.uint8)
        x = np.empty((self.n_groups, self.N_FEATURES), np.float64)
        row_group = np.empty(n, np.int32) if with_row_group else None
        _check(lib.adh_pfdr_read_features(self._s, _p(gpg, C.c_int32), _p(gde, C.c_uint8), _p(x, C.c_double),
                                          _p(row_group, C.c_int32)),
               "adh_pfdr_read_features")
        return (gpg, gde, x, row_group) if with_row_group else (gpg, gde, x)

    def fit_begin(self, x_train, y_train, params) -> None:
        """``adh_pfdr_fit_begin``: the scaled training matrix, its 0 / 1 labels and the 901 initial parameters."""
        x = _abi.as_c(x_train, np.float64)
        y = _abi.as_c(y_train, np.uint8)
        p = _abi.as_c(params, np.float64)
        if x.ndim != 2 or x.shape[1] != self.N_FEATURES or y.shape != (x.shape[0],) or p.shape != (self.N_PARAMS,):
            raise ValueError("fit_begin: x [rows, 7], one label per row, 901 parameters")
        _check(lib.adh_pfdr_fit_begin(self._s, x.shape[0], _p(x, C.c_double), _p(y, C.c_uint8),
                                      _p(p, C.c_double)), "adh_pfdr_fit_begin")
        self.n_train = x.shape[0]

    def epoch(self, order, step_size) -> float:
        """``adh_pfdr_epoch``: one epoch over the rows in ``order``, one Adam step size per batch; the epoch's loss."""
        o = _abi.as_c(order, np.int32)
        lr = _abi.as_c(step_size, np.float64)
        if o.shape != (self.n_train,) or lr.ndim != 1:
            raise ValueError("epoch: one position per training row, one step size per batch")
        loss = C.c_double(0.0)
        _check(lib.adh_pfdr_epoch(self._s, _p(o, C.c_int32), lr.shape[0], _p(lr, C.c_double), C.byref(loss)),
               "adh_pfdr_epoch")
        return float(loss.value)

    def predict(self, x) -> np.ndarray:
        x = _abi.as_c(x, np.float64)
        if x.ndim != 2 or x.shape[1] != self.N_FEATURES:
            raise ValueError("predict: x [rows, 7]")
        out = np.empty(x.shape[0], np.float64)
        _check(lib.adh_pfdr_predict(self._s, x.shape[0], _p(x, C.c_double), _p(out, C.c_double)),
               "adh_pfdr_predict")
        return out

    def gather(self, group_value) -> np.ndarray:
        """``adh_pfdr_gather``: every row's group value, NaN for the rows of no group."""
        v = _abi.as_c(group_value, np.float64)
        if v.shape != (self.n_groups,):
            raise ValueError("gather: one value per group of the last features call")
        out = np.empty(self.n_rows, np.float64)
        _check(lib.adh_pfdr_gather(self._s, v.shape[0], _p(v, C.c_double), _p(out, C.c_double)), "adh_pfdr_gather")
        return out

    def time_ms(self) -> tuple[float, float, float, float]:
        """HIP-event times (ms) of the features, all epochs of the last fit, the last predict and the last gather."""
        return self._times(4, lambda *t: lib.adh_pfdr_time_ms(self._s, *t))


class DeviceTransferLibrary(_DeviceSession):
    """An ``adh_tl_t``: the consensus of the transfer-learning library in HBM - sort keys, dense-row blocks and dense
    matrices - updated run by run (include/alphadia_hip.h: adh_tl_*)."""

    def __init__(self, ctx: Context, n_columns: int, n_matrices: int):
        super().__init__(ctx)
        self.n_columns, self.n_matrices = int(n_columns), int(n_matrices)
        _check(lib.adh_tl_create(ctx._h, self.n_columns, self.n_matrices, C.byref(self._s)), "adh_tl_create")
        self.n_kept = self.n_rows = 0

    def _native_destroy(self, s):
        lib.adh_tl_destroy(s)

    def scatter(self, n_rows: int, row, col, mz, intensity, correlation) -> bool:
        """``adh_tl_scatter``: stages a run from its flat rows; True when a cell was written twice (nothing staged)."""
        r, c = _abi.as_c(row, np.int64), _abi.as_c(col, np.int32)
        v = [_abi.as_c(x, np.float32) for x in (mz, intensity, correlation)]
        if r.ndim != 1 or any(a.shape != r.shape for a in (c, *v)):
            raise ValueError("scatter: one value of every column per flat row")
        dup = C.c_int32(0)
        _check(lib.adh_tl_scatter(self._s, int(n_rows), r.shape[0], _p(r, C.c_int64), _p(c, C.c_int32),
                                  *(_p(a, C.c_float) for a in v), C.byref(dup)), "adh_tl_scatter")
        return bool(dup.value)

    def update(self, keep_top: int, mod_seq_hash, proba, precursor_idx, frag_start, frag_stop, n_new_rows: int,
               matrices=None):
        """``adh_tl_update`` + ``adh_tl_read_kept``: ``(kept, frag_start, frag_stop)`` of the new consensus; ``kept``
        indexes "consensus before the call, then the new run".  ``matrices`` None: the staged run."""
        h = np.ascontiguousarray(mod_seq_hash)
        if h.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
            raise TypeError(f"update: mod_seq_hash must be uint64 or int64, not {h.dtype}")
        pr = np.asarray(proba)
        pr = np.ascontiguousarray(pr, dtype=np.float32 if pr.dtype == np.float32 else np.float64)
        pi, fs, fe = (_abi.as_c(x, np.int64) for x in (precursor_idx, frag_start, frag_stop))
        n = h.shape[0]
        if h.ndim != 1 or any(a.shape != (n,) for a in (pr, pi, fs, fe)):
            raise ValueError("update: one value of every column per precursor")
        mats = None
        if matrices is not None:
            held = [_abi.as_c(m, np.float32) for m in matrices]
            if len(held) != self.n_matrices or any(m.shape != (n_new_rows, self.n_columns) for m in held):
                raise ValueError("update: every dense matrix is [n_new_rows, n_columns]")
            mats = (C.POINTER(C.c_float) * len(held))(*(_p(m, C.c_float) for m in held))
        kept_n, rows_n = C.c_int64(0), C.c_int64(0)
        _check(lib.adh_tl_update(self._s, int(keep_top), n, _p(h), int(h.dtype == np.int64), _p(pr), int(pr.dtype == np.float64),
                                 _p(pi, C.c_int64), _p(fs, C.c_int64), _p(fe, C.c_int64), int(n_new_rows), mats, C.byref(kept_n),
                                 C.byref(rows_n)), "adh_tl_update")
        self.n_kept, self.n_rows = int(kept_n.value), int(rows_n.value)
        kept, start, stop = (np.empty(self.n_kept, np.int64) for _ in range(3))
        _check(lib.adh_tl_read_kept(self._s, _p(kept, C.c_int64), _p(start, C.c_int64), _p(stop, C.c_int64)),
               "adh_tl_read_kept")
        return kept, start, stop

    def matrix(self, m: int) -> np.ndarray:
        """``adh_tl_read_matrix``: dense matrix ``m`` of the consensus."""
        out = np.empty((self.n_rows, self.n_columns), np.float32)
        _check(lib.adh_tl_read_matrix(self._s, int(m), _p(out, C.c_float)), "adh_tl_read_matrix")
        return out

    def time_ms(self) -> tuple[float, float, float]:
        """HIP-event times (ms) of the last update's top-k and row gather and of the last scatter."""
        return self._times(3, lambda *t: lib.adh_tl_time_ms(self._s, *t))


class DeviceMbr(_DeviceSession):
    """An ``adh_mbr_t``: the PSM aggregates, the elution groups that passed and the filtered library of the
    match-between-runs library in HBM (include/alphadia_hip.h: adh_mbr_*)."""

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        _check(lib.adh_mbr_create(ctx._h, C.byref(self._s)), "adh_mbr_create")
        self.n_passed = self.n_by_group = self.n_by_hash = self.n_groups = 0
        self.n_kept = self.n_rows = self.n_columns = 0
        self._rt_dtype = self._hash_dtype = self._group_dtype = None

    def _native_destroy(self, s):
        lib.adh_mbr_destroy(s)

    @staticmethod
    def _group(a, what):
        """The elution-group column as the entry takes it: uint32 as it is, every other integer type as int64."""
        a = np.asarray(a)
        if a.dtype.kind not in "iu" or (a.dtype == np.uint64 and a.size and int(a.max()) >= 2**63):
            raise TypeError(f"{what}: elution_group_idx must be an integer column below 2^63, not {a.dtype}")
        return np.ascontiguousarray(a, dtype=np.uint32 if a.dtype == np.uint32 else np.int64)

    @staticmethod
    def _hash(a, what):
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
            raise TypeError(f"{what}: mod_seq_charge_hash must be uint64 or int64, not {a.dtype}")
        return a

    def aggregate(self, qval, decoy, elution_group_idx, mod_seq_charge_hash, rt_observed, pg_notnull, fdr: float,
                  keep_decoys: bool):
        """``adh_mbr_aggregate``: ``(rows that passed, rows of the table by group, by hash, groups that passed)``."""
        q = np.asarray(qval)
        if q.dtype == np.float32:  # the comparison NumPy makes in float32, restated exactly in float64
            fdr = float(np.float32(fdr))
        q = np.ascontiguousarray(q, dtype=np.float64)
        d = np.asarray(decoy)
        d = np.ascontiguousarray(d).view(np.uint8) if d.dtype.itemsize == 1 else (d != 0).astype(np.uint8)
        eg, h = self._group(elution_group_idx, "aggregate"), self._hash(mod_seq_charge_hash, "aggregate")
        rt = np.asarray(rt_observed)
        rt = np.ascontiguousarray(rt, dtype=np.float32 if rt.dtype == np.float32 else np.float64)
        pg = np.ascontiguousarray(pg_notnull, dtype=np.uint8)
        n = q.shape[0]
        if q.ndim != 1 or any(a.shape != (n,) for a in (d, eg, h, rt, pg)):
            raise ValueError("aggregate: one value of every column per PSM row")
        out = [C.c_int64(0) for _ in range(4)]
        _check(lib.adh_mbr_aggregate(self._s, n, _p(q, C.c_double), _p(d, C.c_uint8), _p(eg), int(eg.dtype == np.uint32), _p(h),
                                     int(h.dtype == np.int64), _p(rt), int(rt.dtype == np.float64), _p(pg, C.c_uint8),
                                     fdr, int(bool(keep_decoys)), *(C.byref(x) for x in out)), "adh_mbr_aggregate")
        self.n_passed, self.n_by_group, self.n_by_hash, self.n_groups = (int(x.value) for x in out)
        self._rt_dtype, self._hash_dtype = rt.dtype, h.dtype
        self._group_dtype = np.asarray(elution_group_idx).dtype
        self.n_kept = self.n_rows = 0
        return self.n_passed, self.n_by_group, self.n_by_hash, self.n_groups

    def table(self, which: int):
        """``adh_mbr_read_table``: ``(keys, median, first pg row)`` of the table by group (0) or by hash (1); the keys
        in the dtype the PSM column had."""
        n = (self.n_by_group, self.n_by_hash)[which]
        keys = np.empty(n, np.int64 if which == 0 else self._hash_dtype)
        med, first = np.empty(n, self._rt_dtype), np.empty(n, np.int64)
        _check(lib.adh_mbr_read_table(self._s, int(which), _p(keys), _p(med), _p(first, C.c_int64)), "adh_mbr_read_table")
        return (keys.astype(self._group_dtype) if which == 0 else keys), med, first

    def groups(self) -> np.ndarray:
        """The elution groups that passed, ascending."""
        keys = np.empty(self.n_groups, np.int64)
        _check(lib.adh_mbr_read_table(self._s, 2, _p(keys), None, None), "adh_mbr_read_table")
        return keys.astype(self._group_dtype)

    def filter(self, elution_group_idx, frag_start, frag_stop, n_rows: int, matrices=None, source_rows: bool = False):
        """``adh_mbr_filter`` + ``adh_mbr_read_filter``: ``(kept, frag_start, frag_stop, source_row)`` - the kept library
        rows, their renumbered blocks and, with ``source_rows``, the old dense row of every kept dense row.
        ``matrices`` None: nothing is gathered on the device."""
        eg = self._group(elution_group_idx, "filter")
        fs, fe = _abi.as_c(frag_start, np.int64), _abi.as_c(frag_stop, np.int64)
        n = eg.shape[0]
        if eg.ndim != 1 or fs.shape != (n,) or fe.shape != (n,):
            raise ValueError("filter: one value of every column per precursor")
        mats, n_cols, held = None, 0, []
        if matrices is not None:
            held = [_abi.as_c(m, np.float32) for m in matrices]
            if not 1 <= len(held) <= _abi.TL_MAX_MATRICES:
                raise ValueError(f"filter: 1 to {_abi.TL_MAX_MATRICES} dense matrices, not {len(held)}")
            if any(m.ndim != 2 or m.shape != held[0].shape or m.shape[0] != n_rows for m in held):
                raise ValueError("filter: every dense matrix is [n_rows, n_columns]")
            n_cols = held[0].shape[1]
            mats = (C.POINTER(C.c_float) * len(held))(*(_p(m, C.c_float) for m in held))
        kept_n, rows_n = C.c_int64(0), C.c_int64(0)
        _check(lib.adh_mbr_filter(self._s, n, _p(eg), int(eg.dtype == np.uint32), _p(fs, C.c_int64), _p(fe, C.c_int64),
                                  int(n_rows), int(n_cols), len(held), mats, C.byref(kept_n), C.byref(rows_n)), "adh_mbr_filter")
        self.n_kept, self.n_rows, self.n_columns = int(kept_n.value), int(rows_n.value), int(n_cols)
        kept, start, stop = (np.empty(self.n_kept, np.int64) for _ in range(3))
        src = np.empty(self.n_rows, np.int64) if source_rows else None
        if self.n_kept:
            _check(lib.adh_mbr_read_filter(self._s, _p(kept, C.c_int64), _p(start, C.c_int64),
                                           _p(stop, C.c_int64), _p(src, C.c_int64)),
                   "adh_mbr_read_filter")
        return kept, start, stop, src

    def matrix(self, m: int) -> np.ndarray:
        """``adh_mbr_read_matrix``: gathered dense matrix ``m`` of the last filter."""
        out = np.empty((self.n_rows, self.n_columns), np.float32)
        if self.n_kept:
            _check(lib.adh_mbr_read_matrix(self._s, int(m), _p(out, C.c_float)), "adh_mbr_read_matrix")
        return out

    def assign(self, elution_group_idx, mod_seq_charge_hash):
        """``adh_mbr_assign``: ``(rt, pg row in the PSM table or -1, precursors whose elution group is missing)``."""
        eg, h = self._group(elution_group_idx, "assign"), self._hash(mod_seq_charge_hash, "assign")
        if h.dtype != self._hash_dtype:
            raise TypeError(f"assign: mod_seq_charge_hash is {h.dtype} in the library and {self._hash_dtype} in the PSM table")
        n = eg.shape[0]
        if eg.ndim != 1 or h.shape != (n,):
            raise ValueError("assign: one value of every column per precursor")
        rt, row, missing = np.empty(n, self._rt_dtype), np.empty(n, np.int64), C.c_int64(0)
        _check(lib.adh_mbr_assign(self._s, n, _p(eg), int(eg.dtype == np.uint32), _p(h), int(h.dtype == np.int64), _p(rt),
                                  _p(row, C.c_int64), C.byref(missing)), "adh_mbr_assign")
        return rt, row, int(missing.value)

    def index(self, target_keys, lookup_keys):
        """``adh_mbr_index``: ``(position of every target in lookup_keys or -1, a lookup key occurs twice)``; both
        columns in an order-preserving uint64 form."""
        t, k = _abi.as_c(target_keys, np.uint64), _abi.as_c(lookup_keys, np.uint64)
        out, dup = np.empty(t.shape[0], np.int64), C.c_int32(0)
        _check(lib.adh_mbr_index(self._s, t.shape[0], _p(t, C.c_uint64), k.shape[0], _p(k, C.c_uint64),
                                 _p(out, C.c_int64), C.byref(dup)), "adh_mbr_index")
        return out, bool(dup.value)

    def stats(self) -> dict:
        """HIP-event times (ms) of the last aggregate, filter, gather and assign; bytes over PCIe since creation."""
        t = [C.c_double(0.0) for _ in range(4)]
        b = [C.c_uint64(0), C.c_uint64(0)]
        _check(lib.adh_mbr_stats(self._s, *(C.byref(x) for x in t), *(C.byref(x) for x in b)), "adh_mbr_stats")
        return dict(aggregate_ms=t[0].value, filter_ms=t[1].value, gather_ms=t[2].value, assign_ms=t[3].value,
                    h2d_bytes=int(b[0].value), d2h_bytes=int(b[1].value))


_contexts: dict[int, Context] = {}


def default_device() -> int:
    return int(os.environ.get("LOCAL_RANK", "0"))


def get_context(device: int | None = None) -> Context:
    """Process-wide context per GPU (so the staged run survives between batches)."""
    device = default_device() if device is None else int(device)
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = Context(device)
        _contexts[device] = ctx
    return ctx
