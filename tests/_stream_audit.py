"""Stream-order audit: a record of what a piece of program enqueues, and a checker that every cross-stream hazard in it is ordered.

record() logs, in enqueue order,
  * launches: every public callable of the two operator modules (wrapped by attribute replacement; reads / writes from ROLES, one row per
    operator) and everything torch itself launches (a TorchDispatchMode; reads / writes from the operator schema), each with the stream
    that was current and the byte range its strides reach for every operand;
  * order edges: Stream.wait_stream / wait_event, Event.record / wait (an event carries the clock of its record, not later work);
  * host synchronisation: Event.synchronize, Stream.synchronize, torch.cuda.synchronize and blocking device-to-host reads;
  * lifetimes: the stream a storage was first seen under, Tensor.record_stream calls, and its death -- logged as a write of the whole
    storage on the allocating stream, because that is whose later work the caching allocator hands the block to.
The recorder keeps numbers and weak references only, launches nothing and synchronises nothing.

hazards(log) replays the log with one vector clock per stream and one for the host.  Two accesses conflict when they sit on different
timelines, their byte ranges intersect and one of them writes; a conflict the earlier of which does not happen-before the later is a
hazard.  The log is a plain list of Entry tuples, so the host tests write logs by hand and the negative controls edit recorded ones."""
import collections
import contextlib
import functools
import importlib
import inspect
import types
import weakref

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

OPS_MODULES = ("4dflownet_amd.ops", "4dflownet_amd.ops_bf16")
HOST = "host"                          # the host's timeline (streams are named by their handle, torch.cuda.Stream.cuda_stream)
DEV, PIN = "dev", "pinned"             # address spaces: device memory, pinned host memory

Access = collections.namedtuple("Access", "operand space lo hi")
# kind: "launch" | "host" (the host touches pinned memory) | "free" | "wait_stream" (stream waits for `other`) | "record" (event `other` on
# stream) | "wait_event" (stream waits for event `other`) | "sync_event" (host waits for event `other`) | "sync_stream" | "sync_device".
# "free": other = the streams named by record_stream for that storage.
Entry = collections.namedtuple("Entry", "seq kind stream name reads writes other")
Pair = collections.namedtuple("Pair", "first second first_operand second_operand kind space lo hi ordered")

# ---------------------------------------------------------------------------------------------------------------- role table
R, W, RW, SHAPE = "r", "w", "rw", "shape"          # SHAPE: a tensor whose shape alone is used
# One row per operator (the function's __name__; a name bound in both modules is one function or two of one signature, tests/test_abi.py),
# one item per parameter that can hold a tensor or a list of tensors.  A tensor met in a parameter that its row does not name fails the
# recording, and the host tests hold the rows against the modules' signatures: every other parameter must be in NOT_TENSORS.
ROLES = {
    "input_features": dict(u=R, v=R, w=R, mu=R, mv=R, mw=R, phase=W, pc=W),
    "input_features_volume": dict(frames=R, phase=W, pc=W),
    "unrotate_accumulate": dict(pred=R, acc=RW),
    "kspace_downsample": dict(vel=R, mag=R, noise=R, out=W, workspace=RW),
    "stitch_patches": dict(pred=R, vol=W, frame_scale=R),
    "blend_patches": dict(pred=R, acc=RW),
    "finish_volume": dict(acc=R, frame_scale=R, out=W),
    "pack_patch_cores": dict(pred=R, out=W),
    "pack_conv64_weights": dict(w=R, wp_fwd=W, wp_dgrad=W),
    "pack_conv64_weights_batch": dict(w_flat=R, w_offsets=R, packs=W),
    "new_sign_mask": dict(y=SHAPE),
    "conv3d_fwd": dict(x=R, w=R, bias=R, residual=R, x2=R, wpack=R, out=W, mask=W),
    "conv64_fwd": dict(x=R, wpack=R, bias=R, residual=R, out=W, mask=W),
    "conv3d_dgrad": dict(dz=R, w=R, wpack_dgrad=R, out=W),
    "conv_cout1_dgrad_folded": dict(dz=R, w=R, y_prev=R, out=W, dbias_prev=W, workspace=RW, mask=R),
    "fold_halo": dict(dxpads=R, skip=R, y_prev=R, out=W),
    "conv3d_dgrad_fused": dict(dz=R, wpack_dgrad=R, dxpad=W, out=W, skip=R, y_prev=R, mask=R),
    "conv3d_dgrad_fused_multi": dict(dzs=R, wpacks_dgrad=R, dxpad=W, out=W, skip=R, y_prev=R, mask=R),
    "fold_halo_border": dict(dxpads=R, out=RW, skip=R, y_prev=R),
    "conv1x1_dgrad": dict(dz=R, w=R, ya=R, yb=R, dxa=W, dxb=W),
    "conv3d_wgrad": dict(x=R, dz=R, x2=R, dw=W, dbias=W, workspace=RW),
    "conv3d_wgrad_batch": dict(xs=R, dzs=R, dws=W, dbiases=W, workspace=RW),
    "upsample_trilinear_fwd": dict(x=R, out=W),
    "upsample_trilinear_bwd": dict(dy=R, y_prev=R, out=W),
    "loss_metrics": dict(pred=R, uh=R, vh=R, wh=R, mask=R, out=W, dpred=W, scratch=RW),
    "volume_metrics": dict(pred=R, truth=R, mask=R, out=W, scratch=RW),
    "l2_sumsq": dict(w_flat=R, is_kernel=R, out=W),
    "l2_sumsq_partials": dict(w_flat=R, is_kernel=R, partials=W),
    "adam_step": dict(w=RW, g=R, m=RW, v=RW, is_kernel=R, l2_scale_dev=R, sumsq_partials=W, lr_t_dev=R, frozen=R, g_scale_dev=R, ema=RW),
    "grad_accumulate": dict(acc=RW, g=R),
    "grad_sumsq_partials": dict(g=R, w=R, is_kernel=R, l2_scale_dev=R, partials=W, frozen=R),
    "clip_scale": dict(partials=R, out=W),
    "sum_partials": dict(partials=R, out=W),
    # queries and argument checks: no operand
    "self_ensemble_orientations": {}, "kspace_crops": {}, "kspace_workspace_bytes": {}, "conv64_mask_ok": {}, "conv64_dgrad_multi_ok": {},
    "wgrad_workspace_bytes": {}, "wgrad_batch_workspace_bytes": {}, "conv64_wgrad_batch_ok": {}, "checked_loss_kind": {},
    "volume_metrics_scratch_doubles": {}, "conv64_pack_streams": {},
}
# every parameter of the operators that is never a tensor (sizes, flags, scalars, host arrays, names)
NOT_TENSORS = frozenset("""patch_size counts g0 count stride orientation first divisor shape crop_ratio nvol crops venc snr_db seed stream_id
    mag_scale side stride_hr want_dgrad N D H W algo act alpha ldy y_coff lddz dz_coff spatial parts algos K Cin Cout want_bias n_layers R
    kind kind_param who error want_grad div_weight non_fluid_weight out_act F lr_t b1 b2 eps l2_grad_scale clip_value ema_momentum
    ema_init clip_norm streams role self_ensemble""".split())


class AuditError(AssertionError):
    pass


def public_callables(mod):
    """name -> function for every public callable an operator module defines or re-exports from the other one."""
    return {n: f for n, f in vars(mod).items()
            if not n.startswith("_") and isinstance(f, types.FunctionType) and f.__module__ in OPS_MODULES}


# ---------------------------------------------------------------------------------------------------------------- checker
def _kind(first_writes, second_writes):
    return "WAW" if first_writes and second_writes else ("RAW" if first_writes else "WAR")


def conflicts(log):
    """Every pair of accesses of `log` on different timelines whose byte ranges intersect with at least one write, as Pair tuples with
    .ordered = the earlier entry happens-before the later one."""
    clocks, events, stamped = {}, {}, []            # stamped: (entry, timeline, tick, clock at the entry)

    def clk(t):
        return clocks.setdefault(t, {})

    def merge(dst, src):
        for k, v in src.items():
            if dst.get(k, 0) < v:
                dst[k] = v

    for e in log:
        if e.kind in ("launch", "free"):            # an enqueue: behind what its stream holds and what the host has done so far
            c = clk(e.stream)
            merge(c, clk(HOST))
            c[e.stream] = c.get(e.stream, 0) + 1
            stamped.append((e, e.stream, c[e.stream], dict(c)))
        elif e.kind == "host":
            c = clk(HOST)
            c[HOST] = c.get(HOST, 0) + 1
            stamped.append((e, HOST, c[HOST], dict(c)))
        elif e.kind == "wait_stream":
            merge(clk(e.stream), clk(HOST))
            merge(clk(e.stream), clk(e.other))
        elif e.kind == "record":                    # the snapshot: what the stream holds NOW
            snap = dict(clk(e.stream))
            merge(snap, clk(HOST))
            events[e.other] = snap
        elif e.kind == "wait_event":                # (an event never recorded: the wait returns at once)
            merge(clk(e.stream), clk(HOST))
            merge(clk(e.stream), events.get(e.other, {}))
        elif e.kind == "sync_event":
            merge(clk(HOST), events.get(e.other, {}))
        elif e.kind == "sync_stream":
            merge(clk(HOST), clk(e.stream))
        elif e.kind == "sync_device":
            for t in list(clocks):
                if t != HOST:
                    merge(clk(HOST), clocks[t])
        else:
            raise ValueError("unknown log entry kind %r" % (e.kind,))

    accs = []                                       # (space, lo, hi, writes, index into stamped, operand)
    for i, (e, _, _, _) in enumerate(stamped):
        for a in e.reads or ():
            accs.append((a.space, a.lo, a.hi, False, i, a.operand))
        for a in e.writes or ():
            accs.append((a.space, a.lo, a.hi, True, i, a.operand))
    accs.sort(key=lambda a: (a[0], a[1]))
    pairs, seen, active = [], set(), []
    for a in accs:
        active = [b for b in active if b[0] == a[0] and b[2] > a[1]]
        for b in active:
            if not (a[3] or b[3]) or a[4] == b[4]:
                continue
            (x, y) = (a, b) if a[4] < b[4] else (b, a)                  # x: the earlier-enqueued one
            ex, tx, tickx, _ = stamped[x[4]]
            ey, ty, _, vcy = stamped[y[4]]
            if tx == ty:
                continue
            if ey.kind == "free" and tx in (ey.other or ()):
                continue                            # record_stream: the allocator itself waits for what that stream held at the free
            key = (x[4], y[4], x[5], y[5], x[3], y[3])
            if key in seen:
                continue
            seen.add(key)
            pairs.append(Pair(ex, ey, x[5], y[5], _kind(x[3], y[3]), a[0], max(a[1], b[1]), min(a[2], b[2]), vcy.get(tx, 0) >= tickx))
        active.append(a)
    pairs.sort(key=lambda p: (p.first.seq, p.second.seq, p.first_operand, p.second_operand))
    return pairs


def hazards(log):
    """The violating pairs of `log`: conflicts whose earlier access does not happen-before the later one."""
    return [p for p in conflicts(log) if not p.ordered]


def describe(p):
    def one(e, operand):
        return "%s [%s seq %s, stream %s] operand %s" % (e.name, e.kind, e.seq, e.stream, operand)
    return "%s %s bytes [%#x, %#x): %s  ->  %s%s" % (p.kind, p.space, p.lo, p.hi, one(p.first, p.first_operand),
                                                     one(p.second, p.second_operand), "" if not p.ordered else "  (ordered)")


def report(pairs, limit=20):
    return "\n".join(describe(p) for p in pairs[:limit]) + ("\n... and %d more" % (len(pairs) - limit) if len(pairs) > limit else "")


def numbered(entries):
    """A hand-written log: the entries with seq = their position."""
    return [e._replace(seq=i) for i, e in enumerate(entries)]


def launch(stream, name, reads=(), writes=(), space=DEV):
    """Entry of a hand-written log; reads / writes: (operand, lo, hi) triples."""
    mk = lambda xs: tuple(Access(o, space, lo, hi) for o, lo, hi in xs)
    return Entry(None, "host" if stream == HOST else "launch", stream, name, mk(reads), mk(writes), None)


def free(stream, lo, hi, record_streams=()):
    return Entry(None, "free", stream, "free", (), (Access("storage", DEV, lo, hi),), frozenset(record_streams))


def edge(kind, stream=None, other=None):
    return Entry(None, kind, stream, kind, (), (), other)


# ---- edits of a recorded log (the negative controls)
def without(log, drop):
    """The log without the entries drop(entry) selects."""
    return [e for e in log if not drop(e)]


def deaths_moved_early(log, stream):
    """The log with the death of every storage that a launch on `stream` touches moved to just behind the first such launch: what
    dropping the references at the launch instead of at the join would record."""
    out, moved = list(log), 0
    for f in [e for e in log if e.kind == "free"]:
        lo, hi = f.writes[0].lo, f.writes[0].hi
        for e in log:
            if e.seq >= f.seq:
                break
            if e.kind == "launch" and e.stream == stream and any(a.space == DEV and a.lo < hi and lo < a.hi for a in e.reads + e.writes):
                # the storage alive at e is the one f frees only if no other death of that range lies between the two
                if any(g.kind == "free" and e.seq < g.seq < f.seq and g.writes[0].lo < hi and lo < g.writes[0].hi for g in log):
                    continue
                out.remove(f)
                out.insert(out.index(e) + 1, f)
                moved += 1
                break
    return out, moved


# ---------------------------------------------------------------------------------------------------------------- recorder
_MISSING = object()


def _tensors_in(name, val):
    if isinstance(val, torch.Tensor):
        yield name, val
    elif isinstance(val, (list, tuple)):
        for i, v in enumerate(val):
            if isinstance(v, torch.Tensor):
                yield "%s[%d]" % (name, i), v


class _Mode(TorchDispatchMode):
    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        self.rec._log_aten(func, args, kwargs, out)
        return out


class Recorder:
    def __init__(self, track_cpu=False):
        self.log = []
        self.track_cpu = track_cpu       # host tests: plain CPU tensors are logged like pinned ones
        self._active = False
        self._depth = 0                  # inside an operator wrapper / an edge wrapper
        self._storages = {}              # StorageImpl address -> [allocating stream, lo, hi, set of record_stream streams]
        self._finalizers = []
        self._next_event = 0
        self._patches = []
        self._mode = _Mode(self)

    # ---- numbers of a tensor
    def _stream(self, s=None):
        if s is None:
            if not torch.cuda.is_available():
                return 0
            s = torch.cuda.current_stream()
        return s.cuda_stream

    def _space(self, t):
        if t.is_cuda:
            return DEV
        if t.device.type != "cpu":
            return None
        if self.track_cpu:
            return PIN
        try:
            return PIN if t.is_pinned() else None
        except RuntimeError:
            return None

    def _access(self, operand, t):
        """The smallest and largest byte the strides of t reach (not the whole storage: views of one flat buffer stay apart)."""
        if isinstance(t, np.ndarray):
            if t.size == 0:
                return None
            lo = t.__array_interface__["data"][0]
            return Access(operand, PIN, lo, lo + sum((n - 1) * s for n, s in zip(t.shape, t.strides)) + t.itemsize)
        space = self._space(t)
        if space is None or t.numel() == 0:
            return None
        self._see(t, space)
        lo = t.data_ptr()
        reach = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
        return Access(operand, space, lo, lo + (reach + 1) * t.element_size())

    def _see(self, t, space=None):
        """Lifetime of t's storage: the stream current at first sight, and a finalizer for its death (device storages only)."""
        if (space or self._space(t)) != DEV:
            return
        st = t.untyped_storage()
        key = st._cdata
        if key not in self._storages and st.nbytes():
            self._storages[key] = [self._stream(), st.data_ptr(), st.data_ptr() + st.nbytes(), set()]
            self._finalizers.append(weakref.finalize(st, self._died, key))

    def _died(self, key):
        info = self._storages.pop(key, None)
        if info is not None and self._active:
            self._append("free", info[0], "free", (), (Access("storage", DEV, info[1], info[2]),), frozenset(info[3]))

    def _append(self, kind, stream, name, reads=(), writes=(), other=None):
        self.log.append(Entry(len(self.log), kind, stream, name, tuple(reads), tuple(writes), other))

    # ---- what a test logs itself
    def _accesses(self, items):
        out = []
        for i, t in enumerate(items):
            operand, t = t if isinstance(t, tuple) else ("arg%d" % i, t)
            a = self._access(operand, t)
            if a is not None:
                out.append(a)
        return out

    def host_access(self, name, reads=(), writes=()):
        """The host touches pinned memory: tensors, numpy arrays, or (operand, either) pairs."""
        self._append("host", HOST, name, self._accesses(reads), self._accesses(writes))

    def launch(self, stream, name, reads=(), writes=()):
        """A launch the recorder cannot see (a stand-in for a collective): logged on `stream`, nothing is run."""
        self._append("launch", stream, name, self._accesses(reads), self._accesses(writes))

    def edge(self, kind, stream=None, other=None):
        self._append(kind, stream, kind, other=other)

    def new_event(self):
        self._next_event += 1
        return "event%d" % self._next_event

    # ---- operator modules
    def _log_operator(self, fn, sig, a, kw, ret):
        row = ROLES.get(fn.__name__)
        bound = sig.bind(*a, **kw)
        reads, writes, args_seen = [], [], set()
        for pname, val in bound.arguments.items():
            for operand, t in _tensors_in(pname, val):
                if row is None or pname not in row:
                    raise AuditError("%s.%s: parameter %r holds a tensor and the role table does not name it" % (fn.__module__, fn.__name__, pname))
                args_seen.add(id(t))
                if row[pname] == SHAPE:
                    continue
                acc = self._access(operand, t)
                if acc is not None:
                    if "r" in row[pname]:
                        reads.append(acc)
                    if "w" in row[pname]:
                        writes.append(acc)
        for operand, t in _tensors_in("return", ret if isinstance(ret, (list, tuple)) else (ret,)):
            if id(t) not in args_seen:                      # allocated by the operator: its output
                acc = self._access(operand, t)
                if acc is not None and fn.__name__ != "new_sign_mask":
                    writes.append(acc)
        if fn.__name__ == "volume_metrics" and bound.arguments.get("scratch") is None:     # the partials buffer the module keeps
            hidden = getattr(inspect.getmodule(fn), "_volume_metrics_scratch", {}).get(bound.arguments["pred"].device)
            acc = None if hidden is None else self._access("scratch(module)", hidden)
            if acc is not None:
                reads.append(acc)
                writes.append(acc)
        if reads or writes:
            self._append("launch", self._stream(), fn.__name__, reads, writes)

    def _wrap_operator(self, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*a, **kw):
            if self._depth:                                 # called by another operator: the outermost call is the launch
                return fn(*a, **kw)
            self._depth += 1
            try:
                ret = fn(*a, **kw)
            finally:
                self._depth -= 1
            self._log_operator(fn, sig, a, kw, ret)
            return ret
        return wrapper

    # ---- torch's own launches
    def _log_aten(self, func, args, kwargs, out):
        packet = func.overloadpacket.__name__
        if packet == "record_stream":                       # (logged by the Tensor.record_stream wrapper)
            return
        schema = func._schema
        reads, writes = [], []
        values = list(zip(schema.arguments, args)) + [(s, kwargs[s.name]) for s in schema.arguments if s.name in kwargs]
        outs = list(_tensors_in("out", out if isinstance(out, (list, tuple)) else (out,)))
        rets = list(schema.returns)
        if len(rets) != len(outs):                          # one Tensor[] return (split and its like), or nothing the schema describes
            rets = rets * len(outs) if len(rets) == 1 else [None] * len(outs)
        fresh = [(n, t) for (n, t), r in zip(outs, rets) if r is None or r.alias_info is None]
        if outs and not fresh and all(r.alias_info is not None and not r.alias_info.is_write for r in rets):
            return                                          # a view: nothing is launched
        if packet.startswith("empty") or packet.startswith("new_empty") or packet in ("_pin_memory", "pin_memory", "is_pinned"):
            for _, t in outs:
                self._see(t)                                # an allocation: the storage belongs to the current stream
            return
        sync = packet in ("_local_scalar_dense", "equal", "is_nonzero", "item")
        if not outs and not sync:
            return
        for s, val in values:
            for operand, t in _tensors_in(s.name, val):
                acc = self._access(operand, t)
                if acc is not None:
                    (writes if s.alias_info is not None and s.alias_info.is_write else reads).append(acc)
        for operand, t in fresh:
            acc = self._access(operand, t)
            if acc is not None:
                writes.append(acc)
        if not (reads or writes):
            return
        stream = self._stream()
        self._append("launch", stream, str(func), reads, writes)
        # a device-to-host copy the host waits for: into pageable memory, or without non_blocking
        to_host = [t for _, t in outs if t.device.type == "cpu"]
        if packet in ("copy_", "_to_copy") and to_host and any(a.space == DEV for a in reads):
            nb = kwargs.get("non_blocking", args[2] if packet == "copy_" and len(args) > 2 else False)
            if not nb or not all(self._space(t) == PIN for t in to_host):
                sync = True
        if sync and any(a.space == DEV for a in reads):
            self._append("sync_stream", stream, "sync_stream")

    # ---- install / remove
    def _patch(self, owner, name, new):
        self._patches.append((owner, name, vars(owner).get(name, _MISSING)))
        setattr(owner, name, new)

    def _edge_wrapper(self, orig, log_it, after=False):
        rec = self

        @functools.wraps(orig)
        def wrapper(*a, **kw):
            outer = not rec._depth
            if outer and not after:
                log_it(*a, **kw)
            rec._depth += 1                                 # (Stream.wait_stream is built from record_event and wait_event: one edge)
            try:
                ret = orig(*a, **kw)
            finally:
                rec._depth -= 1
            if outer and after:
                log_it(*a, **kw)
            return ret
        return wrapper

    def _event_id(self, ev):
        i = getattr(ev, "_stream_audit_id", None)
        if i is None:
            i = ev._stream_audit_id = self.new_event()
        return i

    def _install(self):
        S, E, rec = torch.cuda.Stream, torch.cuda.Event, self
        self._patch(S, "wait_stream", self._edge_wrapper(S.wait_stream, lambda s, other: rec.edge("wait_stream", s.cuda_stream, other.cuda_stream)))
        self._patch(S, "wait_event", self._edge_wrapper(S.wait_event, lambda s, ev: rec.edge("wait_event", s.cuda_stream, rec._event_id(ev))))
        self._patch(S, "synchronize", self._edge_wrapper(S.synchronize, lambda s: rec.edge("sync_stream", s.cuda_stream), after=True))
        self._patch(E, "record", self._edge_wrapper(E.record, lambda ev, stream=None: rec.edge("record", rec._stream(stream), rec._event_id(ev))))
        self._patch(E, "wait", self._edge_wrapper(E.wait, lambda ev, stream=None: rec.edge("wait_event", rec._stream(stream), rec._event_id(ev))))
        self._patch(E, "synchronize", self._edge_wrapper(E.synchronize, lambda ev: rec.edge("sync_event", None, rec._event_id(ev)), after=True))
        self._patch(torch.cuda, "synchronize", self._edge_wrapper(torch.cuda.synchronize, lambda *a, **kw: rec.edge("sync_device"), after=True))

        orig_rs = torch.Tensor.record_stream

        def record_stream(t, stream):
            if t.is_cuda:
                rec._see(t)
                info = rec._storages.get(t.untyped_storage()._cdata)
                if info is not None:
                    info[3].add(stream.cuda_stream)
            return orig_rs(t, stream)
        self._patch(torch.Tensor, "record_stream", record_stream)
        for modname in OPS_MODULES:
            mod = importlib.import_module(modname)
            for name, fn in public_callables(mod).items():
                self._patch(mod, name, self._wrap_operator(fn))
        self._active = True

    def _uninstall(self):
        self._active = False
        for owner, name, old in reversed(self._patches):
            if old is _MISSING:
                delattr(owner, name)
            else:
                setattr(owner, name, old)
        self._patches = []
        for f in self._finalizers:
            f.detach()
        self._finalizers = []
        self._storages = {}


@contextlib.contextmanager
def record(track_cpu=False):
    """Log what the body enqueues; yields the Recorder (its .log is what hazards() takes).  Every replaced attribute is put back on exit,
    also on an exception."""
    rec = Recorder(track_cpu)
    try:
        rec._install()
        with rec._mode:
            yield rec
    finally:
        rec._uninstall()


def patched_attributes():
    """(owner, name) of everything record() replaces for its duration -- for the test that it is put back."""
    out = [(torch.cuda.Stream, n) for n in ("wait_stream", "wait_event", "synchronize")]
    out += [(torch.cuda.Event, n) for n in ("record", "wait", "synchronize")] + [(torch.cuda, "synchronize"), (torch.Tensor, "record_stream")]
    for modname in OPS_MODULES:
        mod = importlib.import_module(modname)
        out += [(mod, n) for n in public_callables(mod)]
    return out


def summary(log):
    """Counts of a log for the sanity floors and the design notes."""
    pairs = conflicts(log)
    launches = [e for e in log if e.kind == "launch"]
    # by_wait: ordered pairs whose order is gone once the stream and event waits are (host synchronisation alone does not order them)
    key = lambda p: (p.first.seq, p.second.seq, p.first_operand, p.second_operand, p.kind)
    loose = set(key(p) for p in conflicts(without(log, lambda e: e.kind in ("wait_stream", "wait_event"))) if not p.ordered)
    return dict(by_wait=sum(p.ordered and key(p) in loose for p in pairs), launches=len(launches), streams=len(set(e.stream for e in launches)), frees=sum(e.kind == "free" for e in log),
                host=sum(e.kind == "host" for e in log), conflicts=len(pairs), ordered=sum(p.ordered for p in pairs),
                hazards=sum(not p.ordered for p in pairs))
