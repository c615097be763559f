"""The loop of the GPU-owning process (pipeline.PooledHotPath.run_windows) and its helpers without a device: the pure pieces
of the loop -- how many images leave in a launch, how long it waits, what a window's predictions do on their way back to its
helper -- as tables, and the whole loop end to end with the two device operations replaced: ``launch`` completes at once,
``fetch_predictions`` derives class and probabilities from each record's twelve integers.  Real forked helpers, the golden
samples; the expectation is the same function through ``_collect_lines`` + ``_vote`` in this process."""
import os

import numpy as np
import pytest

from svision_amd import ingest, pipeline
from svision_amd.io import bam
from svision_amd.sample import Sample
from tests import helpers
from tests.test_hash_batch_cpu import _answer

WINDOWS = [("chrA", 0, 150_000), ("chrA", 150_000, 300_000), ("chrA", 300_000, 420_000), ("chrB", 0, 150_000), ("chrB", 150_000, 200_000)]


# ---- the stand-in for the device ----------------------------------------------------------------------------------------------
def stub_predict(records):
    """int32 [n, 12] -> (classes int64 [n], probs float32 [n, 5]): a function of each record alone, so any grouping of the
    images into launches gives every image the same prediction."""
    rec = np.asarray(records, np.int64).reshape(-1, 12)
    raw = (rec[:, :5] * 7 + rec[:, 5:10] * 3 + rec[:, 10:11] + rec[:, 11:12] * 5 + np.arange(5)) % 97 + 1
    probs = (raw / raw.sum(axis=1, keepdims=True)).astype(np.float32)
    return probs.argmax(axis=1).astype(np.int64), probs


class _Ready:
    def query(self):
        return True

    def synchronize(self):
        pass


class _NoStage:
    """What HotPath.__init__ builds in place of the DeviceStage: only the launch sizes are asked of it."""

    def __init__(self, net, batch, device, n_streams=2, use_graph=True, launch_batches=4, lazy=False, memo=None):
        self.sizes = [4 * batch, 2 * batch, batch]


def stub_hot_path(monkeypatch, sample, options, **kw):
    """A PooledHotPath whose launches complete at once; ``hp.groups``: the images of every launch."""
    monkeypatch.setattr(pipeline, "DeviceStage", _NoStage)
    hp = pipeline.PooledHotPath(sample, options, None, device="cpu", **kw)
    hp.groups = []

    def launch(group):
        group.done_event = _Ready()
        hp.groups.append(group.n_images)
        return group

    hp.launch = launch
    hp.fetch_predictions = lambda group: stub_predict(group.records)
    return hp


def one_process(sample, options, windows):
    """{(chrom, start): (vcf, scores, n_sites, n_images, records)} of ``_collect_lines`` + ``_vote`` with the stand-in's predictions."""
    out = {}
    for chrom, start, end in windows:
        lines = pipeline._collect_lines(sample, options, chrom, start, end)
        records = np.asarray([ln.record() for ln in lines], np.int32).reshape(-1, 12)
        classes, probs = stub_predict(records)
        vcf, scores, n_sites, _head, _tail = pipeline._vote(sample, options, chrom, lines, classes, probs, start, end)
        out[(chrom, start)] = (vcf, scores, n_sites, len(lines), records)
    return out


def pooled(hp, windows, **kw):
    try:
        return {(r.chrom, r.start): r for r in hp.run_windows(windows, **kw)}
    finally:
        hp.close()


def _options(**over):
    return helpers.default_options(min_support=3, batch_size=64, bam_path="<resident>", **over)


@pytest.fixture(scope="module")
def expected(oracle_lib):
    return one_process(helpers.golden_sample(50), _options(), WINDOWS)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_the_pool_gives_what_one_process_gives(oracle_lib, expected, monkeypatch):
    hp = stub_hot_path(monkeypatch, helpers.golden_sample(50), _options(), n_workers=3)
    hp.keep_predictions = True
    got = pooled(hp, WINDOWS, rescan=False)
    assert sorted(got) == sorted(expected)
    for key, (vcf, scores, n_sites, n_images, records) in expected.items():
        r = got[key]
        assert (r.vcf, r.scores, r.n_sites, r.n_images) == (vcf, scores, n_sites, n_images), key
        classes, probs = stub_predict(records)                  # the window's records in TSV order
        assert r.classes.dtype == np.int64 and r.probs.dtype == np.float32 and r.probs.shape == (n_images, 5)
        assert np.array_equal(r.classes, classes) and np.array_equal(r.probs, probs), key
        assert r.n_records == vcf.count("\n") and (r.end, r.wid) == (WINDOWS[r.wid][2], WINDOWS.index((r.chrom, r.start, r.end)))
    assert sum(v[3] for v in expected.values()) == 610 == sum(hp.groups)
    assert sum(v[2] for v in expected.values()) == 27
    prof = hp.owner_profile
    assert isinstance(prof, dict) and all(isinstance(v, (int, float)) for v in prof.values())
    assert prof["launch.partial"] >= 1 and prof["helper.collect_s"] > 0 and prof["last_done_at"] >= prof["last_fetch_at"] >= prof["first_launch_at"] > 0
    assert "scan.n" not in prof and "hash.requests" not in prof and "feed.not_ready" not in prof


def test_a_window_that_fails_after_parts_have_left(oracle_lib, expected, monkeypatch):
    """tests/test_gpu_pipeline.py's scenario: the victim's collection raises after more than 96 lines, in parts of 32."""
    want = pooled(stub_hot_path(monkeypatch, helpers.golden_sample(50), _options(), n_workers=3), WINDOWS, rescan=False)
    victim = max(expected, key=lambda k: expected[k][3])
    assert expected[victim][3] > 128
    real, real_detect, current = pipeline.iter_pair_lines, pipeline.detect_window, []

    def detect(options, sample, chrom, start, end, part_num=0):   # the helpers are forked after these patches: they inherit them
        current[:] = [(chrom, start)]
        return real_detect(options, sample, chrom, start, end, part_num)

    def failing(clusters, options):
        n = 0
        for lines in real(clusters, options):
            yield lines
            n += len(lines)
            if current[0] == victim and n > 96:
                raise ValueError("start out of range (-1)")
    monkeypatch.setattr(pipeline, "detect_window", detect)
    monkeypatch.setattr(pipeline, "iter_pair_lines", failing)
    monkeypatch.setattr(pipeline._collect_parts, "__defaults__", (32,))
    hp = stub_hot_path(monkeypatch, helpers.golden_sample(50), _options(), n_workers=3)
    got = pooled(hp, WINDOWS, rescan=False)
    v = got[victim]
    assert (v.vcf, v.scores, v.n_sites, v.n_images) == ("", "", 0, 0) and v.head is None and v.tail is None
    for key, w in want.items():
        if key != victim:
            g = got[key]
            assert (g.vcf, g.scores, g.n_sites, g.n_images, g.head, g.tail, g.edges) == (w.vcf, w.scores, w.n_sites, w.n_images, w.head, w.tail, w.edges)
            assert (g.vcf, g.scores, g.n_sites, g.n_images) == expected[key][:4]


# ---- --hash: the helpers' requests through the owner ----------------------------------------------------------------------------
class _FakeHandle:
    """kernels.HashSeedsHandle from the host aligner's raw lists; not done for the first polls."""
    made = []

    def __init__(self, bases, desc, k, window, device, fail=False):
        self.msg, self.fail, self.polls, self.launches = ("hash", None, k, window, bases, desc), fail, 0, 1
        _FakeHandle.made.append(self)

    def done(self):
        self.polls += 1
        return self.polls > 3

    def result(self):
        if self.fail:
            raise RuntimeError("out of device memory")
        return _answer(self.msg)[2:]


@pytest.mark.parametrize("fail", [False, True], ids=["executor-works", "executor-fails"])
def test_hash_requests_go_through_the_owner(oracle_lib, monkeypatch, fail):
    monkeypatch.delenv("SVX_HASH_BATCH", raising=False)
    windows = [("chrH", 0, 80_000), ("chrH", 80_000, 160_000)]
    table = bam.read_bam(os.path.join(helpers.GOLDEN, "hash_collect.bam"), with_seq=True)
    sample = Sample.with_scan(table, helpers.load_golden_fasta("hash_collect.fa.gz"), 50, helpers.oracle_scan(table, 50))
    want = one_process(sample, _options(hash=True), windows)   # no device, no owner to ask: the host aligner
    assert [want[(c, s)][3] for c, s, _e in windows] == [64, 36]
    _FakeHandle.made = []
    monkeypatch.setattr(pipeline.kernels, "hash_seeds_async", lambda bases, desc, k, window, device, **more: _FakeHandle(bases, desc, k, window, device, fail))
    hp = stub_hot_path(monkeypatch, sample, _options(hash=True), n_workers=2)
    got = pooled(hp, windows, rescan=False)
    for key, w in want.items():
        r = got[key]
        assert (r.vcf, r.scores, r.n_sites, r.n_images) == w[:4], key
    prof = hp.owner_profile
    assert prof["hash.requests"] == 2 and prof["hash.jobs"] == 57 and sorted(len(h.msg[5]) for h in _FakeHandle.made) == [23, 34]
    assert all(h.polls == 4 for h in _FakeHandle.made)            # polled while not done, answered once
    assert prof["hash.failed"] == (2 if fail else 0) and prof["hash.launches"] == 2 and prof["hash.wait_s"] > 0


# ---- a file-driven feed -------------------------------------------------------------------------------------------------------
class _FakeFeed:
    """ingest.ChromosomeFeed's face to the owner loop: chrA is there, chrB arrives once the loop has asked for it in vain
    (or waits for it with nothing else to do)."""

    def __init__(self, parts):
        self.parts, self.ready, self.fresh, self.refused, self.released = parts, {}, [], 0, []
        self._arrive("chrA")

    def _arrive(self, chrom):
        key, sample, meta = self.parts[chrom]
        self.ready[chrom] = (key, sample)
        self.fresh.append((key, chrom, meta))

    def poll(self, block=False):
        if block and "chrB" not in self.ready:
            self._arrive("chrB")
            return True
        return False

    def take_fresh(self):
        out, self.fresh = self.fresh, []
        return out

    def get(self, chrom, block=True, start=None):
        if chrom not in self.ready:
            self.refused += 1
            if self.refused < 3:
                return None, None
            self._arrive(chrom)
        return self.ready[chrom]

    def keys_of(self, chrom):
        return [self.parts[chrom][0]]

    def release(self, chrom):
        self.released.append(chrom)


class _Spy:
    """A helper's connection that remembers what the owner sent."""

    def __init__(self, conn):
        self.conn, self.sent = conn, []

    def send(self, msg):
        self.sent.append(msg)
        self.conn.send(msg)

    def recv(self):
        return self.conn.recv()

    def fileno(self):
        return self.conn.fileno()


def test_a_file_driven_feed(oracle_lib, expected, monkeypatch, tmp_path):
    stream = bam.BamStream(os.path.join(helpers.GOLDEN, "collect_small.bam"), with_seq=False, threads=2)
    tables = list(stream)
    stream.close()
    fasta = helpers.load_golden_fasta()
    slots, parts = ingest._SlotPool(str(tmp_path)), {}
    for n, table in enumerate(tables):                            # one table per chromosome, through a slot as ChromosomeFeed hands it over
        slot = slots.take()
        ingest.put_table(slot, table, False)
        sample = Sample.with_scan(table, fasta, 50, helpers.oracle_scan(table, 50))
        chrom = table.references[int(table.tid[0])]
        parts[chrom] = ("part-%d" % n, sample, ingest.part_meta(slot, table, sample, table.references, table.lengths, 50, False))
    assert sorted(parts) == ["chrA", "chrB"]
    feed = _FakeFeed(parts)
    pool = pipeline.HelperPool(2, _options(), fasta=fasta)      # forked with the reference only: every Sample comes from a slot
    hp = stub_hot_path(monkeypatch, None, _options(), pool=pool, feed=feed)
    spies = hp.conns = [_Spy(c) for c in pool.conns]
    try:
        got = {(r.chrom, r.start): r for r in hp.run_windows(WINDOWS, rescan=False)}
        for key, w in expected.items():
            r = got[key]
            assert (r.vcf, r.scores, r.n_sites, r.n_images) == w[:4], key
        assert hp.owner_profile["feed.not_ready"] >= 1 and feed.refused >= 1
        told = []
        for spy in spies:
            announced = [m for m in spy.sent if m[0] == "chrom"]
            wins = [m for m in spy.sent if m[0] == "win"]
            assert wins and {m[2] for m in wins} == {m[1] for m in announced}          # told of exactly the parts it got windows of
            assert len(announced) == len({m[1] for m in announced})
            assert ["references" in m[2] and "lengths" in m[2] for m in announced] == [True] + [False] * (len(announced) - 1)
            first_win = {k: min(i for i, m in enumerate(spy.sent) if m[0] == "win" and m[2] == k) for k in {m[1] for m in announced}}
            assert all(spy.sent[i - 1][:2] == ("chrom", k) for k, i in first_win.items())  # right in front of its first window of it
            told.append({m[1] for m in announced})
            del spy.sent[:]
        for chrom in ("chrA", "chrB"):
            hp.release(chrom)
            key = parts[chrom][0]
            for spy, t in zip(spies, told):
                assert [m for m in spy.sent if m[1] == key] == ([("drop", key)] if key in t else [])
        assert feed.released == ["chrA", "chrB"]
        hp.release("chrA")                                       # nobody holds it any more: no second drop
        assert all(sum(m == ("drop", "part-0") for m in spy.sent) <= 1 for spy in spies)
    finally:
        hp.conns = pool.conns
        hp.close()


# ---- the pure pieces ----------------------------------------------------------------------------------------------------------
def _size(pending, room=6144, any_inflight=True, collecting=1, windows_left=True, age=0.0):
    granule, cap = pipeline.launch_limits([256, 128, 64], 64, 3)
    assert (granule, cap) == (256, 6144)
    return pipeline.launch_size(pending, cap - room, granule, cap, any_inflight, collecting, windows_left, age)


def test_launch_size_rule():
    assert _size(255) == (0, False)                               # less than a granule, the device busy, more to come, no wait yet
    assert _size(255, age=0.003) == (255, True)
    assert _size(255, age=0.002) == (0, False)                    # "more than 2 ms"
    assert _size(255, any_inflight=False) == (255, True)
    assert _size(255, collecting=0) == (255, True)
    assert _size(256) == (256, False)
    assert _size(700) == (512, False)
    assert _size(700, collecting=0, windows_left=False) == (256, False)
    assert _size(700, collecting=0, windows_left=True) == (512, False)
    assert _size(700, room=300) == (256, False)
    assert _size(700, room=200) == (0, False)
    assert _size(100, any_inflight=False, room=50) == (100, True)   # a partial launch takes all that is pending, whatever the room
    assert _size(100, any_inflight=False, room=0) == (0, False) and _size(0) == (0, False)
    # a stage without a size of 4 batches: the granule is its largest launch
    assert pipeline.launch_limits([128, 64], 64, 3) == (128, 3072) and pipeline.launch_limits([64], 64, 0) == (64, 512)
    assert pipeline.launch_limits([512, 256, 128], 128, 2) == (512, 8192)


def test_wait_timeouts():
    assert pipeline.wait_timeout(True, True, True) == pipeline.wait_timeout(True, False, False) == 0.0005
    assert pipeline.wait_timeout(False, True, True) == 0.002
    assert pipeline.wait_timeout(False, True, False) == pipeline.wait_timeout(False, False, True) == pipeline.wait_timeout(False, False, False) == 0.05


def _chunk(lo, n):
    classes = np.arange(lo, lo + n, dtype=np.int64) % 5
    return classes, np.full((n, 5), 0.2, np.float32) * (1 + np.arange(lo, lo + n, dtype=np.float32))[:, None]


def test_window_predictions_wait_for_the_size_and_close_on_the_total():
    w = pipeline.WindowPredictions(2)
    assert w.ci == 2
    w.add(0, *_chunk(0, 30), keep=True)
    assert w.take() is None                                       # not before "rec": the helper is not reading its pipe
    w.add(30, *_chunk(30, 20), keep=True)
    assert w.take() is None
    w.sized(70)
    classes, probs, last = w.take()                               # both chunks in one message, in launch order
    assert last is False and np.array_equal(classes, _chunk(0, 50)[0]) and np.array_equal(probs, _chunk(0, 50)[1])
    assert w.take() is None                                       # nothing new
    w.add(50, *_chunk(50, 19), keep=True)
    assert w.take()[2] is False
    w.add(69, *_chunk(69, 1), keep=True)
    classes, probs, last = w.take()
    assert last is True and classes.tolist() == [69 % 5] and probs.shape == (1, 5)
    assert w.take() is None
    kept = w.predictions()
    assert np.array_equal(kept[0], _chunk(0, 70)[0]) and np.array_equal(kept[1], _chunk(0, 70)[1])


def test_window_predictions_of_an_empty_and_of_a_failed_window():
    w = pipeline.WindowPredictions(0)
    w.sized(0)
    classes, probs, last = w.take()
    assert last is True and classes.dtype == np.int64 and classes.shape == (0,) and probs.dtype == np.float32 and probs.shape == (0, 5)
    assert w.take() is None
    f = pipeline.WindowPredictions(1)
    f.add(0, *_chunk(0, 32))
    f.fail()                                                      # "rec" with ok False: parts of it have left
    classes, probs, last = f.take()
    assert last is True and classes.shape == (0,) and probs.shape == (0, 5)
    f.add(32, *_chunk(32, 32))                                    # a launch of it that was still in flight
    assert f.take() is None


def test_kept_predictions_come_back_in_window_order():
    w = pipeline.WindowPredictions(0)
    src = _chunk(40, 10)
    w.add(40, *src, keep=True)
    w.add(0, *_chunk(0, 40), keep=True)
    src[0][:] = -1                                                # kept chunks are copies: the group's buffer is reused
    classes, probs = w.predictions()
    assert np.array_equal(classes, _chunk(0, 50)[0]) and np.array_equal(probs, _chunk(0, 50)[1])
    w.add(50, *_chunk(50, 5))                                     # not kept
    assert len(w.predictions()[0]) == 50
    empty = pipeline.WindowPredictions(0).predictions()
    assert empty[0].dtype == np.int64 and empty[0].shape == (0,) and empty[1].dtype == np.float32 and empty[1].shape == (0, 5)
