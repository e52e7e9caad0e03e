"""ShardedStore.join with TWO PROCESSES on one MI355X (coclr_amd/jpeg.py; csrc/jpeg.hip:
coclr_jpeg_store_gather_shards): each rank holds half of the fixtures of tests/golden/jpeg_frames.pt in its own device
Store, exports its bytes and rows through hipIpc, and decodes ALL global ids -- its own frames from its own memory, the
others from its peer's buffers mapped into this process -- bit for bit what one Store holding every pack returns.  Both
ranks run on cuda:0 with gloo as the host channel, as tests/test_gpu_multirank.py does; across real peer GPUs nothing
has run.  The test also prints what hipPointerGetAttributes reports for a mapped buffer (DESIGN.md section 8 records
it): the entry point launches on it only if the runtime vouches for it, so a refusal shows as a failure, not a fault."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _pointer_report(t):
    """hipPointerGetAttributes on the first and last byte of tensor `t`, asked of the runtime this process has loaded."""
    import ctypes as C

    class Attr(C.Structure):
        _fields_ = [("type", C.c_int), ("device", C.c_int), ("devicePointer", C.c_void_p),
                    ("hostPointer", C.c_void_p), ("isManaged", C.c_int), ("allocationFlags", C.c_uint)]

    path = next((line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line), None)
    if path is None:
        return "no libamdhip64 in this process"
    hip = C.CDLL(path)
    hip.hipPointerGetAttributes.argtypes = [C.POINTER(Attr), C.c_void_p]
    hip.hipPointerGetAttributes.restype = C.c_int
    out = []
    for p in (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size() - 1):
        a = Attr()
        rc = hip.hipPointerGetAttributes(C.byref(a), p)
        out.append("rc %d type %d device %d devicePointer %s hostPointer %s isManaged %d flags %d" %
                   (rc, a.type, a.device, "== the pointer" if a.devicePointer == p else hex(a.devicePointer or 0),
                    hex(a.hostPointer or 0), a.isManaged, a.allocationFlags))
    return "; ".join(out)


def _worker(rank, world, port, q):
    report = ""
    try:
        import datetime
        import random
        import sys
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        here = os.path.dirname(os.path.abspath(__file__))
        for p in (here, os.path.dirname(here)):
            if p not in sys.path:
                sys.path.insert(0, p)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        import _jpeg_cases as J
        import _jpeg_window_cases as WC
        from coclr_amd import jpeg

        cases = J.cases()
        order = random.Random(3).sample(range(54), 54)
        store = jpeg.Store(1 << 17, 64)
        store._advance_cursor(5 * rank + 1)                      # the ranks' frames start at different residues
        for i in order[rank::world]:
            store.add(jpeg.pack([J.raw(cases[i])]))
        sh = jpeg.ShardedStore.join(store)
        report = _pointer_report(sh._mapped[0]) + " | rows: " + _pointer_report(sh._mapped[1])
        assert len(sh) == 54 and sh.bases.tolist() == [0, 27] and len(sh._mapped) == 2
        with pytest.raises(ValueError):
            sh.add(jpeg.pack([J.raw(cases[0])]))
        # one Store of this rank's own with every pack in global order: rank 0's packs, then rank 1's
        single = jpeg.Store(1 << 17, 64)
        where = {i: single.add(jpeg.pack([J.raw(cases[i])])) for r in range(world) for i in order[r::world]}
        picks = random.Random(100 + rank).sample(range(54), 54)  # a permutation of this rank's own
        picks += [picks[3], picks[3], picks[50]]
        ids = torch.tensor([where[i] for i in picks])
        assert set(sh.shard_of(ids).tolist()) == {0, 1}
        for budget in (256 << 20, 40000):
            got, status = sh.decode(ids, return_status=True, max_stage_bytes=budget)
            want, want_status = single.decode(ids, return_status=True, max_stage_bytes=budget)
            assert torch.equal(status, want_status) and not bool(status.any())
            assert torch.equal(got.offset, want.offset) and torch.equal(got.height, want.height)
            for k, i in enumerate(picks):
                assert torch.equal(got.frame(k), want.frame(k)), cases[i]["name"]
                assert torch.equal(got.frame(k).cpu(), cases[i]["rgb"]), cases[i]["name"]      # PIL's bytes
        boxed = [(i, b) for i, b in WC.all_boxes() if cases[i]["width"] <= 64][rank::3]
        sel = torch.tensor([where[i] for i, _ in boxed])
        boxes = torch.tensor([b for _, b in boxed], dtype=torch.int64)
        got, status = sh.decode(sel, boxes, return_status=True)
        want, want_status = single.decode(sel, boxes, return_status=True)
        assert len(boxed) > 300 and set(sh.shard_of(sel).tolist()) == {0, 1}
        assert torch.equal(status, want_status) and not bool(status.any()) and torch.equal(got.offset, want.offset)
        assert all(torch.equal(got.frame(k), want.frame(k)) for k in range(len(boxed)))
        torch.cuda.synchronize()
        sh.close()                                               # collective: nobody leaves while a peer can gather
        with pytest.raises(ValueError):
            sh.decode([0])
        assert torch.equal(store.decode([0]).frame(0).cpu(), cases[order[rank]]["rgb"])        # its owner's again
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", report))
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: %s\n%s" % (e, traceback.format_exc()), report))


def test_two_ranks_share_one_sharded_store():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29741, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = [q.get(timeout=240) for _ in procs]
    finally:
        for p in procs:
            p.join(20)
        for p in procs:                                          # stragglers are ended, not waited for
            if p.is_alive():
                p.terminate()
    for rank, msg, report in results:
        print("rank %d: a peer's mapped buffer -> %s" % (rank, report))
    for rank, msg, _ in results:
        assert msg == "ok", "rank %d: %s" % (rank, msg)
