"""The chained plan (k_decode_plan_chain) and the decoder's handle at the ABI, on streams the oracle emitted for a small rounds
collection: per-target chain starts and one start for the whole collection must give, per contig, the destLen, unmatched and
cursors that swsem_decode_contigs_dev gives on the contig's own streams; the filled bytes must be the contigs."""
import numpy as np
import pytest

import _driver
import _orc
from mbgc_amd import binding, synth

pytestmark = pytest.mark.gpu
NAMES = binding.STREAM_NAMES


class Recording:
    """an oracle emitter that notes where every contig's bytes start and end in the target's six streams"""

    def __init__(self, em, log):
        self.em, self.spans = em, []
        log.append(self)

    def process(self, *a, **k):
        self.target = a[5]
        before = [len(self.em.stream(i)) for i in range(6)]
        r = self.em.process(*a, **k)
        self.spans.append((before, [len(self.em.stream(i)) for i in range(6)]))
        return r

    def put(self, which, data): self.em.put(which, data)
    def streams(self): return self.em.streams()


@pytest.fixture(scope="module", params=[0, 1], ids=["32bit", "bit40"])
def encoded(request):
    bit40 = request.param
    base = synth.base_codes(100_000, 21)
    gs = [synth.genome(base, i, 0.015) for i in range(6)]
    g0 = [gs[0]]
    targets = []
    for i, g in enumerate(gs[1:], 1):
        k = 2 + i % 2
        cuts = [0] + [g.size * j // k + 5 * j for j in range(1, k)] + [g.size]
        targets.append([g[cuts[j]:cuts[j + 1]] for j in range(k)])
    targets[1].append(synth.genome(synth.base_codes(7000, 22), 0, 0.0))              # no match
    targets[2].insert(1, gs[2][40:60].copy())                                        # shorter than the k-mer
    targets[4] = [gs[0].copy()]                                                      # identical to G0
    lim = 8_000_000
    o = _orc.OracleMatcher(lim)
    log = []
    po = _orc.emit_params(1, enable40bitReference=bit40)
    res = _driver.encode_rounds(o, lambda: Recording(_orc.OracleEmitter(o, po), log), g0, targets, 3)
    final = {}
    for em in log:                                                                   # (a target matched again got a new emitter: the last one counts)
        final[em.target] = em
    assert sorted(final) == list(range(len(targets)))
    return dict(res=res, targets=targets, log=[final[t] for t in range(len(targets))], ref=o.ref(lim), lim=lim, bit40=bit40)


def dev(a):
    import torch
    t = torch.from_numpy(np.frombuffer(bytes(a) + b"\0" * 64, dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def test_chained_plan_equals_per_contig_decode_and_fills_the_contigs(encoded):
    import torch
    e = encoded
    p = binding.emit_params(1, enable40bitReference=e["bit40"])
    if e["bit40"]:
        assert len(e["res"]["streams"]["mapOff5th"]) > 0
    coll = [dev(e["res"]["streams"][n]) for n in NAMES]
    sizes = [len(e["res"]["streams"][n]) for n in NAMES]
    streams = [(t.data_ptr(), n) for t, n in zip(coll, sizes)]
    locks = np.frombuffer(e["res"]["locks"], dtype="<u8")
    seq_counts = [len(t) for t in e["targets"]]
    # where every target and contig starts in the collection's streams, from the oracle's per-target streams
    tstart, cstart, at = [], [], [0] * 6
    for em in e["log"]:
        tstart.append(list(at))
        for before, after in em.spans:
            cstart.append(([at[i] + before[i] for i in range(6)], [at[i] + after[i] for i in range(6)]))
        s = em.streams()
        at = [at[i] + len(s[NAMES[i]]) for i in range(6)]
    tstart.append(list(at))
    assert at == sizes
    # the per-contig reference: swsem_decode_contigs_dev on a matcher's handle that holds the oracle's final buffer (nothing wrapped)
    contigs = [c for t in e["targets"] for c in t]
    h = binding.SlidingWindowSparseEMMatcher(e["lim"])
    h.write_ref(0, e["ref"])
    dest = torch.zeros(sum(c.size for c in contigs) + 64 * len(contigs), dtype=torch.uint8, device="cuda:0")
    jobs, off, tl = [], 0, [locks[t] for t, n in enumerate(seq_counts) for _ in range(n)]
    for k, c in enumerate(contigs):
        a, b = cstart[k]
        jobs.append(([(coll[i].data_ptr() + a[i], b[i] - a[i]) for i in range(6)], int(tl[k]), dest.data_ptr() + off, c.size))
        off += c.size + 64
    dl, un = h.decode_contigs_dev(p, jobs)
    assert dl.tolist() == [c.size for c in contigs] and (un >= 0).all()
    assert un.tolist() == [int(u) & 0xFFFFFFFF for u in e["res"]["unmatched"]]
    h.close()

    d = binding.Decoder(e["lim"])
    per_target = [(tstart[t], tstart[t + 1], t, 1, True) for t in range(len(seq_counts))]
    single = [(tstart[0], tstart[-1], 0, len(seq_counts), True)]
    plans = {}
    for name, starts in (("single", single), ("per target", per_target)):
        cc, bad = d.plan_chain(p, streams, starts, seq_counts, locks)
        assert bad == -1, name
        for k, c in enumerate(cc):
            assert (c.destLen, c.unmatched) == (int(dl[k]), int(un[k])), (name, k)
            assert list(c.cur) == cstart[k][0], (name, k)
            assert c.litEnd == cstart[k][1][0], (name, k)
        plans[name] = [(c.destLen, c.unmatched, list(c.cur), c.litEnd, c.minSrc, c.maxSrcEnd, c.nrec) for c in cc]
    assert plans["single"] == plans["per target"]
    # the bytes: the oracle's final buffer into the decoder's, then every contig in one fill
    refdev = dev(e["ref"])
    d.load_segments(refdev.data_ptr(), [(1, 1, e["lim"] - 1, 0)])
    offs = np.concatenate([[0], np.cumsum([c.size for c in contigs])]).astype(np.uint64)
    out = torch.zeros(int(offs[-1]) + 64, dtype=torch.uint8, device="cuda:0")
    assert d.fill_range(0, len(contigs), out.data_ptr(), offs) == 0
    assert out[: int(offs[-1])].cpu().numpy().tobytes() == b"".join(c.tobytes() for c in contigs)
    # a chain that does not end on its offsets, a stream that runs out
    wrong = [list(x) for x in tstart]
    wrong[2][3] += 2
    cc, bad = d.plan_chain(p, streams, [(wrong[t], wrong[t + 1], t, 1, True) for t in range(len(seq_counts))], seq_counts, locks)
    assert bad == 1
    short = list(streams)
    short[3] = (streams[3][0], sizes[3] - 1)
    end = list(tstart[-1]); end[3] -= 1
    cc, bad = d.plan_chain(p, short, [(tstart[0], end, 0, len(seq_counts), True)], seq_counts, locks)
    assert bad == 0 and cc[-1].unmatched == -1
    d.close()


def test_matcher_calls_on_a_decoder_handle_are_refused():
    d = binding.Decoder(1 << 20)
    q = synth.genome(synth.base_codes(2000, 1), 0, 0.0)
    for call in (lambda: d.match(q), lambda: d.load_ref(q), lambda: d.load_separator(), lambda: d.emit_batch(binding.emit_params(1), n=1),
                 lambda: d.emit_verify(), lambda: d.ht(), lambda: d.release_lock(5), lambda: d.emit_batch_end()):
        with pytest.raises(binding.SwsemError, match="swsem error -1"):
            call()
    assert d.ref(16).tolist() == [0] * 16                                             # (the buffer is there, zeroed)
    d.close()
