"""Device context and buffers on top of the C ABI (one Context = one GPU + one stream)."""
from __future__ import annotations

import ctypes
import threading
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import check


class DeviceBuffer:
    """A device allocation (or a view into one) owned by a Context."""

    __slots__ = ("ctx", "ptr", "nbytes", "_owner")

    def __init__(self, ctx: "Context", ptr: int, nbytes: int, owner: Optional["DeviceBuffer"] = None):
        self.ctx = ctx
        self.ptr = ptr
        self.nbytes = nbytes
        self._owner = owner

    def view(self, offset: int, nbytes: Optional[int] = None) -> "DeviceBuffer":
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        if offset < 0 or nbytes < 0 or offset + nbytes > self.nbytes:
            raise ValueError("view out of range")
        return DeviceBuffer(self.ctx, self.ptr + offset, nbytes, self._owner or self)

    def upload(self, host: np.ndarray) -> "DeviceBuffer":
        host = np.ascontiguousarray(host)
        if host.nbytes > self.nbytes:
            raise ValueError(f"upload of {host.nbytes} B into a {self.nbytes} B buffer")
        check(self.ctx.lib.slam_upload(self.ctx.handle, self.ptr, host.ctypes.data, host.nbytes))
        return self

    def download(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError(f"download of {out.nbytes} B from a {self.nbytes} B buffer")
        check(self.ctx.lib.slam_download(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self) -> None:
        if self._owner is None and self.ptr:
            check(self.ctx.lib.slam_free(self.ctx.handle, self.ptr))
            self.ptr = 0


class Context:
    """One HIP device + stream.  Raises if libslamhip or a gfx950 GPU is missing."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        check(self.lib.slam_ctx_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device

    def close(self) -> None:
        if self.handle:
            check(self.lib.slam_ctx_destroy(self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def malloc(self, nbytes: int) -> DeviceBuffer:
        p = ctypes.c_void_p()
        check(self.lib.slam_malloc(self.handle, int(nbytes), ctypes.byref(p)))
        return DeviceBuffer(self, p.value or 0, int(nbytes))

    def upload(self, host: np.ndarray) -> DeviceBuffer:
        host = np.ascontiguousarray(host)
        return self.malloc(host.nbytes).upload(host)

    def set_tuning(self, R: int = 0, blocks_per_cu: int = 0, lead_rows: int = 0, lead_chunk: int = 0,
                   tail: int = 0, feed: int = 0, cold: int = 0, chunk: int = 0, queue: int = 0, merge: int = 0) -> None:
        """Experiment knobs of the top-2 search on this context (``slam_bf_set_tuning``); no arguments = shipped plan."""
        knobs = (ctypes.c_int32 * 10)(R, blocks_per_cu, lead_rows, lead_chunk, tail, feed, cold, chunk, queue, merge)
        check(self.lib.slam_bf_set_tuning(self.handle, knobs, 10))

    def set_engine(self, engine: int = 0) -> None:
        """Which engine runs the top-2 search on this context (``slam_bf_set_engine``): 0 = auto (shipped), 1 = the VALU
        popcount kernel, 2 = the matrix-core kernel on 16x16x128 tiles wherever it is eligible, 3 = the matrix-core kernel on
        32x32x64 tiles wherever 2 would be eligible.  Every engine gives the same tables, bit for bit."""
        check(self.lib.slam_bf_set_engine(self.handle, int(engine)))

    def set_mx_feed(self, feed: int = 0) -> None:
        """How the 32x32x64 matrix-core kernel gets its train rows on this context (``slam_bf_set_mx_feed``): 0 = auto
        (shipped), 1 = expanded in the kernel by every query block, 2 = from an image of the train set prepared once per
        search.  Every feed gives the same tables, bit for bit."""
        check(self.lib.slam_bf_set_mx_feed(self.handle, int(feed)))

    def mx_image_bytes(self) -> int:
        """Current size of the context's prepared-image buffer (``slam_bf_mx_image_bytes``), 0 before the first use."""
        n = ctypes.c_int64(-1)
        check(self.lib.slam_bf_mx_image_bytes(self.handle, ctypes.byref(n)))
        return n.value

    def fill_mx_image(self, byte: int) -> None:
        """Fill the prepared-image buffer with ``byte`` (``slam_bf_mx_image_fill``, a hook for tests)."""
        check(self.lib.slam_bf_mx_image_fill(self.handle, int(byte) & 0xFF))

    def pin_train(self, buf: DeviceBuffer, rows: int) -> None:
        """Declare the ``rows`` train rows at ``buf`` fixed (``slam_bf_train_pin``): their FP4 image is built once, and the
        top-2 searches over exactly (``buf``, ``rows``) read it instead of building one per call.  From here to
        ``unpin_train`` the rows may be rewritten only in front of a ``refresh_train``.  At most 8 sets per context."""
        check(self.lib.slam_bf_train_pin(self.handle, buf.ptr, int(rows)))

    def refresh_train(self, buf: DeviceBuffer) -> None:
        """Rebuild the image of a pinned train set after its rows were rewritten in place (``slam_bf_train_refresh``)."""
        check(self.lib.slam_bf_train_refresh(self.handle, buf.ptr))

    def unpin_train(self, buf: DeviceBuffer) -> None:
        """Drop the registration of a pinned train set (``slam_bf_train_unpin``); freeing the buffer does so too."""
        check(self.lib.slam_bf_train_unpin(self.handle, buf.ptr))

    def mx_image_launches(self) -> int:
        """Launches of the image kernel this context has issued so far (``slam_bf_mx_image_launches``, a hook for tests)."""
        n = ctypes.c_int64(-1)
        check(self.lib.slam_bf_mx_image_launches(self.handle, ctypes.byref(n)))
        return n.value

    def train_pins(self) -> int:
        """Train sets this context holds pinned (``slam_bf_train_pins``, a hook for tests)."""
        n = ctypes.c_int64(-1)
        check(self.lib.slam_bf_train_pins(self.handle, ctypes.byref(n)))
        return n.value

    def state_dirty(self) -> int:
        """Words of the search's merge state that are not idle once the stream has drained (``slam_bf_state_dirty``):
        0 after every completed search."""
        n = ctypes.c_int64(-1)
        check(self.lib.slam_bf_state_dirty(self.handle, ctypes.byref(n)))
        return n.value

    BLOCKS = ("workspace", "merge_state", "pinned_block", "io_dev", "io_host", "radius_tables")

    def block_bytes(self) -> dict:
        """Current sizes of the context's grow-only blocks (``slam_ctx_block_bytes``), 0 for a block not yet taken."""
        b = (ctypes.c_int64 * len(self.BLOCKS))()
        check(self.lib.slam_ctx_block_bytes(self.handle, b, len(self.BLOCKS)))
        return dict(zip(self.BLOCKS, b))

    def fill_block(self, name: str, byte: int) -> None:
        """Fill one scratch block with ``byte`` (``slam_ctx_block_fill``, a hook for tests): "workspace", "io_dev", "io_host"
        or "radius_tables".  The blocks that carry state between calls ("merge_state", "pinned_block") are refused."""
        check(self.lib.slam_ctx_block_fill(self.handle, self.BLOCKS.index(name), int(byte) & 0xFF))

    def plan_info(self, n: int, m: int) -> dict:
        """The launch plan the top-2 search would use for n x m (``slam_bf_plan_info``)."""
        p = (ctypes.c_int32 * 10)()
        check(self.lib.slam_bf_plan_info(self.handle, n, m, p))
        return dict(zip(("R", "qblocks", "chunk", "chunks", "lead_rows", "lead_chunks", "tail_chunks", "cus", "sgpr_feed", "cold_rows"), p))

    def sync(self) -> None:
        check(self.lib.slam_sync(self.handle))

    def timer_start(self) -> None:
        check(self.lib.slam_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = ctypes.c_float(0)
        check(self.lib.slam_timer_stop(self.handle, ctypes.byref(ms)))
        return ms.value

    def prof_enable(self, on: bool = True) -> None:
        check(self.lib.slam_prof_enable(self.handle, int(on)))

    def prof_read(self) -> Tuple[int, float]:
        n = ctypes.c_int64(0)
        ms = ctypes.c_double(0)
        check(self.lib.slam_prof_read(self.handle, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value


_default_lock = threading.Lock()
_default_ctx: Optional[Context] = None


def default_context() -> Context:
    """Process-wide context on device 0 (what the drop-in matcher uses)."""
    global _default_ctx
    with _default_lock:
        if _default_ctx is None:
            _default_ctx = Context(0)
        return _default_ctx


PLAN_KNOBS = ("R", "blocks_per_cu", "lead_rows", "lead_chunk", "tail", "feed", "cold", "chunk", "queue", "merge")


def mx_plan_describe(n: int, m: int, num_cu: int = 256):
    """The matrix-core plan of the top-2 search for n x m on a device with ``num_cu`` CUs, WITHOUT a device
    (``slam_bf_mx_plan_describe``): (plan dict, chunk boundary table)."""
    lib = _lib.load()
    plan = (ctypes.c_int32 * 8)()
    cap = 1 << 16
    tbl = (ctypes.c_int32 * cap)()
    length = ctypes.c_int64(0)
    check(lib.slam_bf_mx_plan_describe(num_cu, n, m, plan, tbl, cap, ctypes.byref(length)))
    names = ("qblocks", "workers", "chunk", "chunks", "tail_chunks", "stage_rows", "resident", "auto")
    return dict(zip(names, plan)), list(tbl[:min(length.value, cap)])


def mx_tile_describe(n: int, m: int, engine: int = 0) -> int:
    """Which matrix-core kernel a pass of n x m runs on under ``engine`` (0, 2 or 3), WITHOUT a device
    (``slam_bf_mx_tile_describe``): 16 for the 16x16x128 kernel, 32 for the 32x32x64 kernel."""
    tile = ctypes.c_int32(0)
    check(_lib.load().slam_bf_mx_tile_describe(int(engine), n, m, ctypes.byref(tile)))
    return tile.value


def mx_feed_describe(n: int, m: int, feed: int = 0) -> int:
    """The feed a pass of n x m on the 32x32x64 kernel takes under ``feed`` (0, 1 or 2), WITHOUT a device
    (``slam_bf_mx_feed_describe``): 1 = expanded in the kernel, 2 = from the prepared image."""
    out = ctypes.c_int32(0)
    check(_lib.load().slam_bf_mx_feed_describe(int(feed), n, m, ctypes.byref(out)))
    return out.value


def mx_feed_describe_pinned(n: int, m: int, feed: int = 0) -> int:
    """``mx_feed_describe`` for a pass whose train set is pinned (``slam_bf_mx_feed_describe_pinned``): the image costs such
    a pass no launch, so it is taken at more shapes."""
    out = ctypes.c_int32(0)
    check(_lib.load().slam_bf_mx_feed_describe_pinned(int(feed), n, m, ctypes.byref(out)))
    return out.value


def plan_describe(n: int, m: int, num_cu: int = 256, qb_all: int = 0, rows_on_host: bool = False, **knobs):
    """The launch plan of the top-2 search for n x m on a device with ``num_cu`` CUs, WITHOUT a device
    (``slam_bf_plan_describe``): (plan dict, chunk boundary table).  ``knobs``: as ``Context.set_tuning``."""
    unknown = set(knobs) - set(PLAN_KNOBS)
    if unknown:
        raise TypeError(f"unknown knobs {sorted(unknown)}")
    lib = _lib.load()
    k = (ctypes.c_int32 * len(PLAN_KNOBS))(*(int(knobs.get(name, 0)) for name in PLAN_KNOBS))
    plan = (ctypes.c_int32 * 14)()
    cap = 1 << 16
    tbl = (ctypes.c_int32 * cap)()
    length = ctypes.c_int64(0)
    check(lib.slam_bf_plan_describe(num_cu, k, len(PLAN_KNOBS), n, m, qb_all, int(rows_on_host), plan, tbl, cap, ctypes.byref(length)))
    names = ("R", "qblocks", "chunk", "chunks", "lead_rows", "lead_chunks", "tail_chunks", "cus", "sgpr_feed", "cold_rows",
             "table_free", "bound_free", "workers", "resident")
    out = dict(zip(names, plan))
    out["merge"], out["resident"] = out["resident"] >> 8, out["resident"] & 255
    return out, list(tbl[:min(length.value, cap)])
