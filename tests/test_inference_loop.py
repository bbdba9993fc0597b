"""The streamed evaluation loop (dafne_amd/evaluation/inference.py): the counterpart of detectron2's
inference_on_dataset(model, data_loader, evaluator) as tools/plain_train_net.py:316-336 calls it, with the reference's
DafneEvaluator protocol (dafne/evaluation/dafne_evaluator.py:39-69).  CPU tests with a stub detector (the loop's order /
drain logic, the evaluator's 2-rank gather over gloo); the GPU tests compare the streamed results with forward()'s."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inst(g, k):
    from dafne_amd.structures import Boxes, Instances
    inst = Instances((64, 64))
    inst.pred_corners = torch.full((k, 8), float(g))
    inst.scores = torch.arange(k, 0, -1).float() / 10
    inst.centerness = torch.ones(k)
    inst.pred_classes = torch.full((k,), g, dtype=torch.int64)
    inst.pred_boxes = Boxes(torch.zeros(k, 4))
    return inst


class _StubStreamed:
    """forward_streamed / flush with the engine's contract: a call enqueues its batch and hands back the outputs of the OLDEST
    batch in flight once more than `depth` are (the detector: depth 2), else None; flush() hands out the rest, oldest first,
    one batch per call, then None."""

    def __init__(self, depth=2):
        self.depth = depth
        self.pending = []
        self.calls = []
        self.training = False

    def eval(self):
        return self

    def _run(self, inputs):
        return [{"instances": _inst(x.get("idx", x["image_id"]), x.get("idx", x["image_id"]) % 5 + 1)} for x in inputs]

    def __call__(self, inputs):
        self.calls.append(("sync", [x["image_id"] for x in inputs]))
        return self._run(inputs)

    def forward_streamed(self, inputs):
        self.calls.append(("stream", [x["image_id"] for x in inputs]))
        self.pending.append(self._run(inputs))
        return self.pending.pop(0) if len(self.pending) > self.depth else None

    def flush(self):
        return self.pending.pop(0) if self.pending else None


class _Recorder:
    def __init__(self):
        self.pairs = []

    def reset(self):
        self.pairs = []

    def process(self, inputs, outputs):
        assert len(inputs) == len(outputs)
        self.pairs.extend((x["image_id"], int(o["instances"].pred_classes[0]), len(o["instances"])) for x, o in zip(inputs, outputs))

    def evaluate(self):
        return {"n": len(self.pairs)}


def _loader(n, b, lo=0):
    items = [{"image_id": lo + i, "file_name": "f%d" % (lo + i), "height": 64, "width": 64} for i in range(n)]
    return [items[i:i + b] for i in range(0, n, b)]


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("n,b", [(7, 3), (1, 4), (8, 8), (0, 2), (9, 2)])
def test_streamed_loop_pairs_inputs_with_their_outputs(n, b, depth):
    from dafne_amd.evaluation.inference import inference_on_dataset
    m, ev, stats = _StubStreamed(depth), _Recorder(), {}
    res = inference_on_dataset(m, _loader(n, b), ev, stats)
    assert res == {"n": n} and stats["images"] == n
    assert ev.pairs == [(g, g, g % 5 + 1) for g in range(n)]            # every image once, in order, with ITS outputs
    assert all(c[0] == "stream" for c in m.calls) and m.pending == []   # drained

    class Sync:                                                            # a model without the streamed form (the TTA wrapper)
        def __call__(self, inputs):
            return m._run(inputs)
    ev2 = _Recorder()
    inference_on_dataset(Sync(), _loader(n, b), ev2)
    assert ev2.pairs == ev.pairs
    outs = inference_on_dataset(m, _loader(n, b))                          # no evaluator: the outputs themselves
    assert [int(o["instances"].pred_classes[0]) for o in outs] == list(range(n))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dafne_amd.evaluation.gather import shard_range
    from dafne_amd.evaluation.inference import DafneEvaluator, inference_on_dataset
    ok = True
    for n_total, b in ((7, 3), (1, 2), (6, 2)):              # ragged shards, an EMPTY shard on rank 1, even shards
        lo, hi = shard_range(n_total, rank, world)
        ev = DafneEvaluator("stub", None, distributed=True, k_cap=16, device=torch.device("cpu"), pad_to=(n_total + world - 1) // world)
        res = inference_on_dataset(_StubStreamed(), _loader(hi - lo, b, lo), ev)
        if rank == 0:
            preds = sorted(res["predictions"], key=lambda p: p["image_id"])
            ok = ok and [p["image_id"] for p in preds] == list(range(n_total))
            ok = ok and all(p["labels"].tolist() == [g] * (g % 5 + 1) and float(p["corners"][0, 0]) == g for g, p in enumerate(preds))
            ok = ok and all(p["file_name"] == "f%d" % g and (p["height"], p["width"]) == (64, 64) for g, p in enumerate(preds))
        else:
            ok = ok and res == {}
    # pad_to=None (the default): the ranks agree on the LARGEST local image count by a MAX all-reduce -- ragged contiguous
    # shards (7 = 4 + 3, 1 = 1 + 0) used to hand mismatched shapes to the gather (advisor, round 4) -- and an output WITHOUT
    # "instances" keeps its image's slot (an empty image), so later images do not shift
    class _NoInst(_StubStreamed):
        def _run(self, inputs):
            outs = super()._run(inputs)
            return [({} if x["image_id"] == 2 else o) for x, o in zip(inputs, outs)]
    for n_total, b in ((7, 3), (1, 2)):
        lo, hi = shard_range(n_total, rank, world)
        ev = DafneEvaluator("stub", None, distributed=True, k_cap=16, device=torch.device("cpu"))
        res = inference_on_dataset(_NoInst(), _loader(hi - lo, b, lo), ev)
        if rank == 0:
            preds = sorted(res["predictions"], key=lambda p: p["image_id"])
            ok = ok and [p["image_id"] for p in preds] == list(range(n_total))
            ok = ok and all(p["labels"].tolist() == ([] if g == 2 else [g] * (g % 5 + 1)) for g, p in enumerate(preds))
            ok = ok and all(p["file_name"] == "f%d" % g for g, p in enumerate(preds))
        else:
            ok = ok and res == {}
    # a dataset evaluator (a subclass with _eval_predictions: DotaEvaluator / HrscEvaluator / UcasAodEvaluator) on string image ids
    # (UCAS-AOD's): rank 0 scores ALL images with their own file names, the other ranks return {} (dafne_evaluator.py:60-84)
    class Scoring(DafneEvaluator):
        def _eval_predictions(self, predictions):
            self._results["seen"] = [(p["image_id"], p["file_name"], len(p["scores"])) for p in predictions]
    lo, hi = shard_range(5, rank, world)
    items = [{"image_id": "P%04d" % i, "idx": i, "file_name": "/d/P%04d.png" % i, "height": 64, "width": 64} for i in range(lo, hi)]
    ev = Scoring("stub", None, distributed=True, k_cap=16, device=torch.device("cpu"), pad_to=3)
    res = inference_on_dataset(_StubStreamed(), [items[i:i + 2] for i in range(0, len(items), 2)], ev)
    if rank == 0:
        ok = ok and res == {"seen": [("P%04d" % i, "/d/P%04d.png" % i, i % 5 + 1) for i in range(5)]}
    else:
        ok = ok and res == {}
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


def test_dafne_evaluator_gathers_two_ranks_over_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(r[1] for r in res), res


def test_single_process_evaluator_keeps_the_reference_fields():
    from dafne_amd.evaluation.inference import DafneEvaluator, inference_on_dataset
    ev = DafneEvaluator("stub", None, distributed=False)
    res = inference_on_dataset(_StubStreamed(), _loader(5, 2), ev)
    assert res["num_images"] == 5
    for g, p in enumerate(res["predictions"]):
        assert set(p) == {"image_id", "file_name", "height", "width", "labels", "scores", "corners", "centerness"}   # dafne_evaluator.py:46-57
        assert p["image_id"] == g and p["file_name"] == "f%d" % g and p["labels"].tolist() == [g] * (g % 5 + 1)


def test_the_loop_caps_torchs_thread_pool_and_restores_it():
    """inference_on_dataset owns the cap on torch's intra-op pool (utils.host.capped_torch_threads): inside the loop at most
    min(8, usable_cpus()) threads, afterwards the caller's count again -- the detector used to shrink the pool process-wide and
    for good from inside _pack_inputs (advisor, round 4)."""
    from dafne_amd.evaluation.inference import inference_on_dataset
    from dafne_amd.utils.host import capped_torch_threads, usable_cpus
    before = torch.get_num_threads()
    seen = []

    class Probe(_StubStreamed):
        def forward_streamed(self, inputs):
            seen.append(torch.get_num_threads())
            return super().forward_streamed(inputs)
    torch.set_num_threads(max(before, 2))
    try:
        n0 = torch.get_num_threads()
        inference_on_dataset(Probe(), _loader(5, 2))
        assert seen and all(t <= min(8, usable_cpus()) and t <= n0 for t in seen), (seen, n0)
        assert torch.get_num_threads() == n0
        with capped_torch_threads(1):
            assert torch.get_num_threads() == 1
        assert torch.get_num_threads() == n0
    finally:
        torch.set_num_threads(before)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _gpu_model(cfgname="dota-1.0_r50.yaml", splits=None, seed=11):
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    cfg = load_cfg(os.path.join(ROOT, "configs", cfgname))
    if splits is not None:
        cfg.ENGINE.PIPELINE_SPLITS = splits
    m = build_model(cfg)
    m.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=seed))
    m.to(torch.device("cuda", 0))
    m.invalidate()
    return cfg, m


def _same(a, b):
    ia, ib = a["instances"], b["instances"]
    return (len(ia) == len(ib) and ia.image_size == ib.image_size and torch.equal(ia.pred_corners, ib.pred_corners)
            and torch.equal(ia.scores, ib.scores) and torch.equal(ia.pred_classes, ib.pred_classes)
            and torch.equal(ia.pred_boxes.tensor, ib.pred_boxes.tensor))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_streamed_loop_equals_forward_per_image(where):
    """inference_on_dataset over 7 images of three sizes, one image per batch (detectron2's test loader) and in batches of
    2 with ONE sub-batch stream: every image's streamed result EQUALS model([input]) / model(batch) -- same kernels on the
    same batch composition; only the enqueue order and the streams differ.  Host images go through the pinned staging."""
    from dafne_amd.evaluation.inference import inference_on_dataset
    cfg, m = _gpu_model(splits=1)
    g = torch.Generator().manual_seed(4)
    sizes = [(128, 160), (128, 160), (96, 224), (128, 160), (160, 128), (96, 224), (128, 160)]
    items = []
    for i, (h, w) in enumerate(sizes):
        img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
        items.append({"image": img.cuda() if where == "device" else img, "height": h + 7, "width": w + 3, "image_id": i})
    for b in (1, 2):
        loader = [items[i:i + b] for i in range(0, len(items), b)]
        expected = [o for batch in loader for o in m(batch)]
        torch.cuda.synchronize()
        stats = {}
        got = inference_on_dataset(m, loader, None, stats)
        assert len(got) == len(items) and stats["images"] == len(items)
        assert all(len(o["instances"]) > 0 for o in got)
        for i, (a, e) in enumerate(zip(got, expected)):
            assert _same(a, e), (b, i, len(a["instances"]), len(e["instances"]))
        assert m.flush() is None


@pytest.mark.gpu
def test_streamed_outputs_carry_a_host_twin():
    """forward_streamed copies a batch's packed rows to pinned host memory behind its NMS; the Instances it hands out live on the
    device (as forward()'s do) and `.to("cpu")` -- the reference's evaluators call it per image, dafne_evaluator.py:48-55 -- returns
    Instances built from that copy: equal, field by field, to the device-to-host copy of the same Instances."""
    from dafne_amd.evaluation.inference import inference_on_dataset
    cfg, m = _gpu_model()
    g = torch.Generator().manual_seed(33)
    items = [{"image": torch.randint(0, 256, (3, 128, 160), generator=g, dtype=torch.uint8).cuda(), "height": 135, "width": 163, "image_id": i}
             for i in range(10)]
    got = inference_on_dataset(m, [items[i:i + 4] for i in range(0, 10, 4)])
    assert len(got) == 10
    for o in got:
        inst = o["instances"]
        assert inst.scores.is_cuda and inst.__dict__.get("_cpu_twin") is not None
        twin = inst.to(torch.device("cpu"))
        assert len(twin) == len(inst) > 0 and twin.image_size == inst.image_size
        for name, v in inst.get_fields().items():
            w = twin.get(name)
            a, b = (v.tensor, w.tensor) if hasattr(v, "tensor") else (v, w)
            assert not b.is_cuda and b.dtype == a.dtype and torch.equal(a.cpu(), b), name


@pytest.mark.gpu
def test_single_image_batches_rotate_streams_and_plan_sets():
    """The reference's own loop shape -- ONE image per call (tools/plain_train_net.py:316-336, tools/benchmark.py:117-145) -- through
    inference_on_dataset: consecutive calls run on alternating compute streams and four plan sets (forward_streamed, round 5), so
    the convolutions of up to three images are in flight at once.  13 different images of one shape, large enough for the calls
    to overlap: every image's result EQUALS model([input]); repeated with the rotation off (same results again)."""
    from dafne_amd.evaluation.inference import inference_on_dataset
    cfg, m = _gpu_model()
    g = torch.Generator().manual_seed(21)
    items = [{"image": torch.randint(0, 256, (3, 512, 640), generator=g, dtype=torch.uint8).cuda(), "height": 512, "width": 640, "image_id": i}
             for i in range(13)]
    expected = [m([it])[0] for it in items]
    torch.cuda.synchronize()
    assert not torch.equal(expected[0]["instances"].scores, expected[1]["instances"].scores)          # the images really differ
    for rep in range(2):
        got = inference_on_dataset(m, [[it] for it in items])
        assert len(got) == len(items)
        bad = [i for i, (a, e) in enumerate(zip(got, expected)) if not _same(a, e)]
        if bad:          # which side moved?  (a failure message that tells a wrong first call from a wrong streamed call)
            again = [m([it])[0] for it in items]
            torch.cuda.synchronize()
            raise AssertionError("rep %d: streamed != model([input]) for images %s; model([input]) repeated equals its first run: %s; "
                                 "streamed equals the repeated run: %s" % (rep, bad, [_same(a, e) for a, e in zip(again, expected)],
                                                                            [_same(a, e) for a, e in zip(got, again)]))
        assert m.flush() is None
    pipe = [st for key, st in m._pipe.items() if key[0] == 1]
    assert pipe and len(pipe[0]["plans"]) == 4                       # four plan sets for the unsplittable batch


@pytest.mark.gpu
def test_streamed_loop_on_the_benchmarked_layout():
    """The default layout (ENGINE.PIPELINE_SPLITS 3, unequal sub-batches: bench.py's): batches of 8 through forward_streamed give exactly what
    detect_packed(pipelined=True, splits=3) gives for the same batch (the call bench.py times), in order, and EXACTLY what
    model(batch) gives (round 5: forward() of >= 2 images runs on the same sub-batch layout; an image gets the same bits in
    any batch composition anyway)."""
    from dafne_amd import postprocess as pp
    from dafne_amd.evaluation.inference import inference_on_dataset
    cfg, m = _gpu_model()
    assert cfg.ENGINE.PIPELINE_SPLITS == 3
    g = torch.Generator().manual_seed(9)
    items = [{"image": torch.randint(0, 256, (3, 128, 160), generator=g, dtype=torch.uint8), "height": 128, "width": 160, "image_id": i}
             for i in range(24)]
    loader = [items[i:i + 8] for i in range(0, 24, 8)]
    got = inference_on_dataset(m, loader)
    assert len(got) == 24
    for k, batch in enumerate(loader):
        bd = torch.stack([x["image"] for x in batch]).cuda()
        rows, counts = m.detect_packed(bd, pipelined=True, splits=3)
        torch.cuda.synchronize()
        direct = pp.rows_to_instances(rows, counts, [(128, 160)] * 8)
        for i in range(8):
            assert _same(got[8 * k + i], {"instances": direct[i]}), (k, i)
        sync = m(batch)                          # round 5: forward() itself runs >= 2 images on sub-batch streams
        for i in range(8):
            assert _same(got[8 * k + i], sync[i]), (k, i)
    # the streamed loop: three sub-batches of unequal size; the synchronous call: two equal ones (a lone step ends with its longest stream)
    assert m._pipe[(8, 128, 160, 3)]["bounds"] == [0, 3, 5, 8] and m._pipe[(8, 128, 160, 2, "even")]["bounds"] == [0, 4, 8]


@pytest.mark.gpu
def test_graph_replay_equals_eager_launches(monkeypatch):
    """ENGINE.HIP_GRAPHS (default on): from a plan set's second use the pipelined step replays every sub-batch's dense
    launches from a HIP graph (one host call per stream instead of ~200).  Same kernels, same arguments, same buffers:
    the detections are bit-identical to the eagerly launched step, call after call (both plan sets, graph capture in the
    middle of the sequence)."""
    cfg, m = _gpu_model()
    assert cfg.ENGINE.HIP_GRAPHS
    g = torch.Generator().manual_seed(21)
    batches = [torch.randint(0, 256, (8, 3, 128, 160), generator=g, dtype=torch.uint8).cuda() for _ in range(6)]
    monkeypatch.setenv("DAFNE_HIP_GRAPHS", "0")
    eager = []
    for b in batches:
        r, c = m.detect_packed(b, pipelined=True, splits=3)
        torch.cuda.synchronize()
        eager.append((r.clone(), c.clone()))
    st = m._pipe[(8, 128, 160, 3)]
    assert all(p.graph is None for ps in st["plans"] for p in ps)
    monkeypatch.setenv("DAFNE_HIP_GRAPHS", "1")
    for b, (r0, c0) in zip(batches, eager):
        r, c = m.detect_packed(b, pipelined=True, splits=3)
        torch.cuda.synchronize()
        assert torch.equal(c, c0)
        for i in range(8):
            assert torch.equal(r[i, :int(c0[i])], r0[i, :int(c0[i])])
    assert all(p.graph is not None for ps in st["plans"] for p in ps)          # both plan sets were captured and replayed


@pytest.mark.gpu
def test_graph_capture_survives_runtime_calls_of_other_threads():
    """A multi-process job has threads that call the HIP runtime while the main thread captures its launch plans (RCCL's
    watchdog polling events, a loader staging the next batch in pinned memory).  The plans are captured with thread-local
    error checking (engine._CAPTURE_MODE): a capture-unsafe call elsewhere -- here pinned allocations, device allocations
    and event queries in a loop -- neither breaks the capture nor changes the replayed results."""
    import threading
    from dafne_amd import engine
    assert engine._CAPTURE_MODE == "thread_local"
    cfg, m = _gpu_model()
    g = torch.Generator().manual_seed(33)
    batches = [torch.randint(0, 256, (4, 3, 128, 160), generator=g, dtype=torch.uint8).cuda() for _ in range(6)]
    ref = []
    for b in batches:
        r, c = m.detect_packed(b, pipelined=True, splits=2, graphs=False)
        torch.cuda.synchronize()
        ref.append((r.clone(), c.clone()))
    m.invalidate()                                                             # fresh plan sets: the captures below are new
    stop, errs = threading.Event(), []

    def noise():
        try:
            torch.cuda.set_device(0)
            side = torch.cuda.Stream()
            k = 0
            while not stop.is_set():
                k += 1
                h = torch.empty(4096 << (k % 12), dtype=torch.uint8).pin_memory()     # new size classes: hipHostMalloc, capture-unsafe
                with torch.cuda.stream(side):                                         # under the default ("global") checking
                    d = h.to("cuda", non_blocking=True)
                    e = torch.cuda.Event()
                    e.record(side)
                while not e.query():
                    pass
                e.synchronize()
                del h, d
        except Exception as ex:                                                # pragma: no cover
            errs.append(ex)

    th = threading.Thread(target=noise, daemon=True)
    th.start()
    try:
        for b, (r0, c0) in zip(batches, ref):
            r, c = m.detect_packed(b, pipelined=True, splits=2, graphs=True)
            torch.cuda.synchronize()
            assert torch.equal(c, c0)
            for i in range(4):
                assert torch.equal(r[i, :int(c0[i])], r0[i, :int(c0[i])])
    finally:
        stop.set()
        th.join(timeout=30)
    assert not errs, errs
    st = m._pipe[(4, 128, 160, 2)]
    assert all(p.graph is not None for ps in st["plans"] for p in ps)


@pytest.mark.gpu
@pytest.mark.parametrize("graphs", [False, True])
def test_deferred_post_process_gives_the_step_results_one_call_later(graphs):
    """detect_packed(defer=True): call i enqueues its convolutions, then the decode + NMS of call i - 1 (started where call i's
    sub-batches reach their head towers), and returns call i - 1's results; flush_deferred() the last.  Same bits as the
    immediate form on the same batches -- eager launches and the two-part HIP graphs -- also across a change of shape and
    with an immediate call in between."""
    cfg, m = _gpu_model(splits=2)
    declared = set(vars(m))
    g = torch.Generator().manual_seed(31)
    dev = torch.device("cuda", 0)
    batches = [torch.randint(0, 256, (4, 3, 128, 160), generator=g, dtype=torch.uint8).to(dev) for _ in range(5)]
    batches.insert(3, torch.randint(0, 256, (4, 3, 96, 224), generator=g, dtype=torch.uint8).to(dev))       # another plan set
    want = []
    for b in batches:
        r, c = m.detect_packed(b, pipelined=True, splits=2, graphs=graphs)
        torch.cuda.synchronize()
        want.append((r.clone(), c.clone()))
    assert m.flush_deferred() is None
    for rep in range(2):                                   # second pass: graphs are captured and replayed
        got = []
        for b in batches:
            res = m.detect_packed(b, pipelined=True, splits=2, graphs=graphs, defer=True)
            if res is not None:
                got.append(res)
        assert len(got) == len(batches) - 1
        got.append(m.flush_deferred())
        assert m.flush_deferred() is None
        torch.cuda.synchronize()
        for i, ((r, c), (rw, cw)) in enumerate(zip(got, want)):
            assert torch.equal(c, cw), (rep, i)
            assert all(torch.equal(r[k, :int(cw[k])], rw[k, :int(cw[k])]) for k in range(4)), (rep, i)
    # an immediate call while a deferred step is pending: the pending one is completed first and stays retrievable
    assert m.detect_packed(batches[0], pipelined=True, splits=2, graphs=graphs, defer=True) is None
    r1, c1 = m.detect_packed(batches[1], pipelined=True, splits=2, graphs=graphs)
    r0, c0 = m.flush_deferred()
    torch.cuda.synchronize()
    assert torch.equal(c0, want[0][1]) and torch.equal(c1, want[1][1])
    assert torch.equal(r0[0, :int(c0[0])], want[0][0][0, :int(c0[0])]) and torch.equal(r1[0, :int(c1[0])], want[1][0][0, :int(c1[0])])
    with pytest.raises(ValueError):
        m.detect_packed(batches[0], defer=True)
    # every piece of runtime state is declared at construction (none is created on first use), and invalidate() empties it
    assert set(vars(m)) == declared
    assert m.detect_packed(batches[0], pipelined=True, splits=2, graphs=graphs, defer=True) is None
    torch.cuda.synchronize()
    m.invalidate()                                         # drops the pending step with its plans
    assert m.flush_deferred() is None and m.flush() is None
    assert set(vars(m)) == declared
