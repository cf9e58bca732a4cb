"""The stream-order checker on hand-written logs, the role table against the operator modules, and the recorder's dispatch mode on CPU
tensors.  No device: the GPU side is tests/test_gpu_stream_audit.py."""
import gc
import importlib
import inspect
import weakref

import pytest
import torch

import _stream_audit as A
from _stream_audit import HOST, PIN, edge, free, launch, numbered

S1, S2, S3 = 1, 2, 3
X = ("x", 0, 100)


def found(entries):
    return {(p.first.seq, p.second.seq, p.kind) for p in A.hazards(numbered(entries))}


@pytest.mark.parametrize("kind,first,second,span", [("RAW", dict(writes=[X]), dict(reads=[("x", 50, 60)]), (50, 60)),
                                                    ("WAR", dict(reads=[X]), dict(writes=[("x", 99, 200)]), (99, 100)),
                                                    ("WAW", dict(writes=[X]), dict(writes=[X]), (0, 100))])
def test_two_streams_with_and_without_the_wait(kind, first, second, span):
    a, b = launch(S1, "a", **first), launch(S2, "b", **second)
    assert found([a, b]) == {(0, 1, kind)}
    assert found([a, edge("wait_stream", S2, S1), b]) == set()
    assert found([edge("wait_stream", S2, S1), a, b]) == {(1, 2, kind)}        # a wait taken before the earlier launch orders nothing
    assert found([a, edge("wait_stream", S1, S2), b]) == {(0, 2, kind)}        # nor does the wait the other way round
    (p,) = A.hazards(numbered([a, b]))
    assert (p.first.name, p.second.name, p.first.stream, p.second.stream, p.first_operand, p.second_operand) == ("a", "b", S1, S2, "x", "x")
    assert (p.lo, p.hi) == span
    assert "a [launch seq 0, stream 1] operand x" in A.describe(p) and "b [launch seq 1, stream 2]" in A.describe(p)


def test_order_carried_through_a_third_stream():
    a, b = launch(S1, "a", writes=[X]), launch(S2, "b", reads=[X])
    assert found([a, edge("wait_stream", S3, S1), edge("wait_stream", S2, S3), b]) == set()
    assert found([a, edge("wait_stream", S2, S3), edge("wait_stream", S3, S1), b]) == {(0, 3, "RAW")}      # S2 took S3's clock too early


def test_an_event_carries_the_snapshot_of_its_record():
    a, b = launch(S1, "a", writes=[X]), launch(S2, "b", reads=[X])
    assert found([edge("record", S1, "e"), a, edge("wait_event", S2, "e"), b]) == {(1, 3, "RAW")}          # recorded before the writer
    assert found([a, edge("record", S1, "e"), edge("wait_event", S2, "e"), b]) == set()
    assert found([a, edge("wait_event", S2, "never recorded"), b]) == {(0, 2, "RAW")}
    # a second record moves the event; the wait sees the latest one
    assert found([edge("record", S1, "e"), a, edge("record", S1, "e"), edge("wait_event", S2, "e"), b]) == set()


def test_read_read_same_stream_and_disjoint_views_are_silent():
    assert found([launch(S1, "a", reads=[X]), launch(S2, "b", reads=[X])]) == set()
    assert found([launch(S1, "a", writes=[X]), launch(S1, "b", writes=[X], reads=[X])]) == set()
    # two views of one storage [0, 200): [0, 100) and [100, 200) touch at a byte boundary and do not intersect
    assert found([launch(S1, "a", writes=[("buf[:25]", 0, 100)]), launch(S2, "b", writes=[("buf[25:]", 100, 200)])]) == set()
    assert found([launch(S1, "a", writes=[("buf[:25]", 0, 101)]), launch(S2, "b", writes=[("buf[25:]", 100, 200)])]) == {(0, 1, "WAW")}
    # device and pinned memory are address spaces of their own
    assert found([launch(S1, "a", writes=[X]), launch(S2, "b", writes=[X], space=PIN)]) == set()


def test_a_death_is_a_write_on_the_allocating_stream():
    """x is allocated under S1 and read by a launch on S2.  Freed before S1 has waited for S2, S1's later work may be handed the block."""
    use = [launch(S1, "producer", writes=[X]), edge("wait_stream", S2, S1), launch(S2, "reader", reads=[X])]
    assert found(use + [free(S1, 0, 100)]) == {(2, 3, "WAR")}
    assert found(use + [edge("wait_stream", S1, S2), free(S1, 0, 100)]) == set()                          # after the join
    assert found(use + [free(S1, 0, 100, record_streams=[S2])]) == set()                                  # the allocator waits itself
    assert found(use + [free(S1, 0, 100, record_streams=[S3])]) == {(2, 3, "WAR")}                        # (another stream's does not help)
    # record_stream covers what S2 held at the death, not what it is given afterwards
    late = launch(S2, "late reader", reads=[X])
    assert found(use + [free(S1, 0, 100, record_streams=[S2]), late]) == {(3, 4, "RAW")}
    assert found(use + [free(S1, 0, 100, record_streams=[S2]), edge("wait_stream", S2, S1), late]) == set()
    (p,) = A.hazards(numbered(use + [free(S1, 0, 100)]))
    assert p.second.kind == "free" and p.second_operand == "storage" and p.first.name == "reader"


def test_the_host_is_a_timeline_of_its_own():
    a, b = launch(S2, "copy", writes=[X]), launch(S1, "reader", reads=[X])
    assert found([a, b]) == {(0, 1, "RAW")}
    assert found([a, edge("record", S2, "e"), edge("sync_event", None, "e"), b]) == set()                  # enqueued after the host waited
    assert found([edge("record", S2, "e"), a, edge("sync_event", None, "e"), b]) == {(1, 3, "RAW")}
    assert found([a, edge("sync_stream", S2), b]) == set()
    assert found([a, edge("sync_stream", S3), b]) == {(0, 2, "RAW")}
    assert found([a, edge("sync_device"), b]) == set()
    # pinned slot: written by a copy on S2, read by the host, written again by the next copy
    slot = ("slot", 0, 64)
    d2h, read = launch(S2, "d2h", writes=[slot], space=PIN), launch(HOST, "on_host", reads=[slot], space=PIN)
    assert found([d2h, read]) == {(0, 1, "RAW")}
    assert found([d2h, edge("record", S2, "e"), edge("sync_event", None, "e"), read, d2h]) == set()         # the later copy is behind the host
    # ring slot: filled by the host, read by a copy on S2, refilled
    fill, h2d = launch(HOST, "fill", writes=[slot], space=PIN), launch(S2, "h2d", reads=[slot], space=PIN)
    assert found([fill, h2d, fill]) == {(1, 2, "WAR")}                                                    # refilled while the copy is in flight
    assert found([fill, h2d, edge("record", S2, "e"), edge("sync_event", None, "e"), fill]) == set()


def test_log_edits_of_the_negative_controls():
    log = numbered([launch(S1, "dgrad", writes=[X]), edge("wait_stream", S2, S1), launch(S2, "wgrad", reads=[X], writes=[("g", 500, 600)]),
                    edge("wait_stream", S1, S2), free(S1, 0, 100), launch(S1, "adam", reads=[("g", 500, 600)])])
    assert A.hazards(log) == []
    assert A.summary(log)["ordered"] == 3 and A.summary(log)["streams"] == 2 and A.summary(log)["by_wait"] == 3
    synced = numbered([launch(S1, "a", writes=[X]), edge("sync_device"), launch(S2, "b", reads=[X])])
    assert A.summary(synced)["ordered"] == 1 and A.summary(synced)["by_wait"] == 0          # ordered by the host alone
    no_wait = A.without(log, lambda e: e.kind == "wait_stream" and (e.stream, e.other) == (S2, S1))
    assert {(p.first.name, p.second.name, p.kind) for p in A.hazards(no_wait)} == {("dgrad", "wgrad", "RAW")}
    no_join = A.without(log, lambda e: e.kind == "wait_stream" and (e.stream, e.other) == (S1, S2))
    assert {(p.first.name, p.second.name, p.kind) for p in A.hazards(no_join)} == {("wgrad", "free", "WAR"), ("wgrad", "adam", "RAW")}
    early, moved = A.deaths_moved_early(log, S2)
    assert moved == 1 and [e.name for e in early][2:4] == ["wgrad", "free"]
    assert {(p.first.name, p.second.name, p.kind) for p in A.hazards(early)} == {("wgrad", "free", "WAR")}


# ---------------------------------------------------------------------------------------------------------------- role table
def test_role_table_names_every_public_callable_and_every_parameter():
    """Every public callable of both operator modules has a row, and every parameter of it is either named by the row (it can hold a
    tensor) or is one of the names that never do: a new operator or a new tensor parameter cannot slip past the recorder."""
    names = set()
    for modname in A.OPS_MODULES:
        mod = importlib.import_module(modname)
        fns = A.public_callables(mod)
        assert len(fns) >= 25, (modname, sorted(fns))
        for name, fn in fns.items():
            names.add(fn.__name__)
            assert fn.__name__ in A.ROLES, "%s.%s has no row in the role table" % (modname, name)
            row = A.ROLES[fn.__name__]
            params = list(inspect.signature(fn).parameters)
            assert set(row) <= set(params), (modname, name, sorted(set(row) - set(params)))
            for p in params:
                assert (p in row) != (p in A.NOT_TENSORS), "%s.%s: parameter %r must be in the row or in NOT_TENSORS, not %s" % (
                    modname, name, p, "both" if p in row else "neither")
            assert all(r in (A.R, A.W, A.RW, A.SHAPE) for r in row.values())
    assert names == set(A.ROLES), sorted(set(A.ROLES) - names)             # no row for an operator that is gone
    # the operators a train step reaches, by name: both modules offer them
    for modname in A.OPS_MODULES:
        mod = importlib.import_module(modname)
        for n in ("conv3d_fwd", "conv3d_wgrad", "conv3d_wgrad_batch", "conv3d_dgrad_fused", "conv3d_dgrad_fused_multi", "fold_halo_border",
                  "conv_cout1_dgrad_folded", "loss_metrics", "adam_step", "pack_conv64_weights_batch"):
            assert n in A.public_callables(mod), (modname, n)


# ---------------------------------------------------------------------------------------------------------------- recorder
def _attribute_state():
    return [vars(owner).get(name, None) for owner, name in A.patched_attributes()]


def test_record_puts_every_replaced_attribute_back():
    before = _attribute_state()
    assert len(before) > 60
    with A.record(track_cpu=True):
        inside = _attribute_state()
        assert all(a is not b for a, b in zip(before, inside))
        ops = importlib.import_module("4dflownet_amd.ops")
        assert ops.conv64_dgrad_multi_ok([0, 0]) is True                   # a wrapped query still answers, and logs nothing
    assert all(a is b for a, b in zip(before, _attribute_state()))
    assert "record_stream" not in vars(torch.Tensor)
    with pytest.raises(KeyError):
        with A.record(track_cpu=True):
            raise KeyError("from the body")
    assert all(a is b for a, b in zip(before, _attribute_state()))
    t = torch.ones(3)
    t.add_(1)                                                              # the dispatch mode is gone too
    assert t.tolist() == [2.0, 2.0, 2.0]


def test_dispatch_mode_on_cpu_tensors():
    """In-place, view and out-of-place operations with known reads and writes; CPU tensors stand in for pinned ones (track_cpu)."""
    with A.record(track_cpu=True) as rec:
        a = torch.zeros(8)                       # float32: 32 bytes
        b = a[2:6]                               # a view: no launch
        b.add_(1.0)                              # writes bytes [8, 24) of a
        c = a.double()                           # reads a, writes c
        d = torch.empty(8)                       # an allocation: no launch
        d.copy_(a)                               # reads a, writes d
        e = a[::2] + b                           # reads a strided view (bytes [0, 28)) and b
        pa, pc_, pd, pe = a.data_ptr(), c.data_ptr(), d.data_ptr(), e.data_ptr()
        ref = weakref.ref(c)
        del c
        gc.collect()
        assert ref() is None                     # the recorder holds no reference to what it has logged
    log = rec.log
    assert [x.kind for x in log] == ["launch"] * 5
    spans = lambda accs: sorted((x.lo, x.hi) for x in accs)
    names = [x.name for x in log]
    assert names[0].startswith("aten.zeros") and names[1].startswith("aten.add_") and names[2].startswith("aten._to_copy")
    assert names[3].startswith("aten.copy_") and names[4].startswith("aten.add.")
    assert spans(log[0].writes) == [(pa, pa + 32)] and not log[0].reads
    assert spans(log[1].writes) == [(pa + 8, pa + 24)]
    assert spans(log[2].reads) == [(pa, pa + 32)] and spans(log[2].writes) == [(pc_, pc_ + 64)]
    assert spans(log[3].reads) == [(pa, pa + 32)] and spans(log[3].writes) == [(pd, pd + 32)]
    assert spans(log[4].reads) == [(pa, pa + 28), (pa + 8, pa + 24)] and spans(log[4].writes) == [(pe, pe + 16)]
    assert all(x.space == PIN for e_ in log for x in e_.reads + e_.writes) and all(e_.stream == 0 for e_ in log)
    assert [x.seq for x in log] == list(range(5))
    assert A.hazards(log) == []                  # one timeline


def test_an_unnamed_tensor_argument_fails_the_recording(monkeypatch):
    ops = importlib.import_module("4dflownet_amd.ops")
    monkeypatch.setitem(A.ROLES, "kspace_crops", {})

    def kspace_crops(shape, crop_ratio):         # an operator that has grown a tensor parameter the table does not know
        return None
    kspace_crops.__module__ = ops.__name__
    monkeypatch.setattr(ops, "kspace_crops", kspace_crops)
    with A.record(track_cpu=True):
        ops.kspace_crops((4, 4, 4), 0.5)
        with pytest.raises(A.AuditError, match="role table does not name"):
            ops.kspace_crops(torch.zeros(3), 0.5)


def test_operator_wrappers_log_the_outermost_call_only(monkeypatch):
    ops = importlib.import_module("4dflownet_amd.ops")

    def sum_partials(partials, out=None):        # stands for a launcher: calls another public operator inside
        ops.clip_scale(partials, 1.0, out)
        return out

    def clip_scale(partials, clip_norm, out=None):
        return out
    for f in (sum_partials, clip_scale):
        f.__module__ = ops.__name__
        monkeypatch.setattr(ops, f.__name__, f)
    with A.record(track_cpu=True) as rec:
        p, o = torch.zeros(4), torch.zeros(2)
        n0 = len(rec.log)
        ops.sum_partials(p, o)
        ops.clip_scale(p[1:3], 1.0, o)
    mine = rec.log[n0:]
    assert [e.name for e in mine] == ["sum_partials", "clip_scale"]
    assert [(a.operand, a.lo - p.data_ptr(), a.hi - p.data_ptr()) for a in mine[0].reads] == [("partials", 0, 16)]
    assert [(a.operand, a.lo - p.data_ptr(), a.hi - p.data_ptr()) for a in mine[1].reads] == [("partials", 4, 12)]
    assert [a.operand for a in mine[0].writes] == ["out"]


def test_the_module_scratch_of_volume_metrics_is_an_operand(monkeypatch):
    """volume_metrics keeps its per-block partials in a buffer on the module when no scratch is passed: the recorder logs it."""
    ops = importlib.import_module("4dflownet_amd.ops")

    def volume_metrics(pred, truth, mask, out=None, scratch=None):           # the signature of the operator, nothing launched
        return out
    volume_metrics.__module__ = ops.__name__
    assert list(inspect.signature(ops.volume_metrics).parameters) == list(inspect.signature(volume_metrics).parameters)
    monkeypatch.setattr(ops, "volume_metrics", volume_metrics)
    pred, truth, mask, out, kept, own = (torch.zeros(4) for _ in range(6))
    monkeypatch.setattr(ops, "_volume_metrics_scratch", {pred.device: kept})
    with A.record(track_cpu=True) as rec:
        n0 = len(rec.log)
        ops.volume_metrics(pred, truth, mask, out)
        ops.volume_metrics(pred, truth, mask, out, own)
    a, b = rec.log[n0:]
    assert [(x.operand, x.lo) for x in a.writes] == [("out", out.data_ptr()), ("scratch(module)", kept.data_ptr())]
    assert ("scratch(module)", kept.data_ptr()) in [(x.operand, x.lo) for x in a.reads]
    assert [(x.operand, x.lo) for x in b.writes] == [("out", out.data_ptr()), ("scratch", own.data_ptr())]
    monkeypatch.delattr(ops, "_volume_metrics_scratch")                      # a module without the buffer: nothing hidden, no error
    with A.record(track_cpu=True) as rec:
        ops.volume_metrics(pred, truth, mask, out)
    assert [x.operand for x in rec.log[-1].writes] == ["out"]
