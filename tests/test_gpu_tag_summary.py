"""The summary of the lap tags (RefView::tagSum): one entry per 2^SWSEM_TAGSUM_SHIFT sampling slots that says
"every slot of this block holds this tag" or "mixed: look at the tags". The resolve kernels settle a stale table entry from
it where they can, so it may only ever claim what tags[] holds, and nothing that is computed may depend on it.

  invariant   after every round of a run through more than three laps of a small circular buffer (separators after every
              target, an off-grid stretch after every wrap) every
              block the summary calls uniform holds that tag in all of its slots — and, at 16 slots per block, most blocks
              are uniform, as the loader's own piece arithmetic (restated below) says they must be
  exactness   match rows, the six streams and the table image are the same round by round with the summary off (shift 0,
              which is also held to the oracle as test_gpu_laps.py does), at 4, 6 and the default 12
  taken back  a speculative finalize that is not applied leaves the summary of a handle that never speculated
  sequential  one chain per wave (SWSEM_CHAINS=1) and K above the four-chain kernel's limit (k_resolve_blocks, k_stitch)

The switch is read when a handle is made, so a run sets it in this process's environment around the handle's creation."""
import contextlib
import functools
import hashlib
import os

import numpy as np
import pytest

import _driver
import _orc
import _spec
from mbgc_amd import synth

pytestmark = pytest.mark.gpu
LIM = 2_400_000
N_GENOMES, GENOME = 86, 100_000          # 85 targets of 100 kbp, each loaded whole with its separator: 3.5 laps of LIM
MIXED = 0xFFFF
SHIFTS = (0, 4, 6, 12)
# Share of uniform blocks asserted at shift 4 once the buffer has been written all over (piece_blocks has the arithmetic): a
# 100 kbp piece touches 391 or 392 blocks of 256 bytes and its on-grid main run covers all but the ~2 KB the samples lag behind
# the text at either end, the tail's samples and the separator: 371 at least. One piece per lap (24 pieces) follows a wrap,
# samples off the grid and has none. 371 / 392 * 23 / 24 = 0.907; the piece the loader is in the middle of and the first
# file's reverse complement (loaded by a kernel of its own, same arithmetic) leave that untouched. Asked for: 0.85.
UNIFORM_SHARE = 0.85


@contextlib.contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make(max_ref, shift, **kw):
    from mbgc_amd import binding
    assert binding.lib().swsem_device_count() > 0, "no HIP device: the GPU tests must run on the MI355X box"
    env = {"SWSEM_TAGSUM_SHIFT": shift, "SWSEM_CHAINS": kw.pop("chains", None), "SWSEM_LAP_TAGS": None, "SWSEM_RESOLVE": None}
    with environment(**env):
        h = binding.SlidingWindowSparseEMMatcher(max_ref, **kw)
    s, sh = h.tag_summary()
    assert sh == shift and (s.size > 0) == (shift > 0)
    return h


def digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()


def check_invariant(h, what):
    """-> (uniform blocks, blocks). Every block the summary calls uniform holds that tag in every slot."""
    s, sh = h.tag_summary()
    t = h.tags()
    assert s.size == ((t.size - 1) >> sh) + 1, what
    padded = np.zeros(s.size << sh, dtype=np.uint16)
    padded[: t.size] = t
    blocks = padded.reshape(s.size, 1 << sh)
    uni = s != MIXED
    bad = np.nonzero(uni & (blocks != s[:, None]).any(axis=1))[0]
    assert bad.size == 0, "%s: %d blocks of the summary claim a tag their slots do not all hold, the first %d (summary %d, tags %r)" % (
        what, bad.size, bad[0], s[bad[0]], blocks[bad[0]])
    return int(uni.sum()), int(s.size)


def piece_blocks(lo, n, sampling_pos, K, k1=16, shift=4):
    """The loader's arithmetic (processIgnoreCollisionsRef's two sample sets) for a piece of n bytes written at lo while the
    sampling position stands at sampling_pos, on the grid: -> (blocks the piece touches, blocks its main run covers whole)."""
    step = k1 * 128
    E = lo + n - K
    n_main = (((E - step) - sampling_pos + step - 1) // step) * 128 if sampling_pos < E - step else 0
    a, b = sampling_pos // k1, sampling_pos // k1 + n_main                      # slots of the main run
    per = 1 << shift
    whole = max(0, b // per - (a + per - 1) // per)
    touched = ((lo + n - 1) // k1) // per - (max(lo - K + 1, 0) // k1) // per + 1
    return touched, whole


def test_the_piece_arithmetic_gives_the_share_asked_for():
    """no GPU work: the bound the device is held to below follows from the loader's arithmetic for these inputs"""
    worst = 1.0
    for lo in (1, 300_017, 2_000_000 + 255, 1_234_567):
        for lag in (0, 16 * 128 - 16, 16 * 128 + 48):                             # how far the sampling position trails the text
            sp = (lo - lag) // 16 * 16 if lo > lag else 16
            touched, whole = piece_blocks(lo, GENOME, sp, 28)
            assert touched in (391, 392) and whole >= 371, (lo, lag, touched, whole)
            worst = min(worst, whole / touched)
    pieces_per_lap = LIM // (GENOME + 1)
    assert pieces_per_lap == 23 and worst * (pieces_per_lap - 1) / pieces_per_lap >= UNIFORM_SHARE + 0.04


def collection():
    base = synth.base_codes(GENOME, 71)
    return [synth.genome(base, i, 0.01) for i in range(N_GENOMES)]


@functools.lru_cache(maxsize=None)
def rounds_run(shift, round_size=1):
    """the collection through RoundRunner (speculative finalizes included) at one shift: -> per round the digests of the match
    rows, of what the streams grew by, of the table image; the final streams; the share of uniform blocks at the end"""
    import torch
    from mbgc_amd import binding
    from mbgc_amd.rounds import RoundRunner, round_schedule
    gs = collection()
    h = make(LIM, shift)
    h.set_sliding_window_size(16)
    h.load_ref(gs[0], load_rc=True)
    runner = RoundRunner(h, 0, 1, None, "cuda:0", lazy=True, emit_params=binding.emit_params(1))
    runner.start()
    recs, seen, laps, share = [], {k: 0 for k in runner.streams}, 0, None
    last_pos = h.loading_position()
    for r, rnd in enumerate(round_schedule(len(gs) - 1, round_size, 1)):
        mine = [gs[1 + t] for t in rnd[0]]
        buf = torch.from_numpy(np.concatenate(mine)).to("cuda:0")
        offs = np.zeros(len(mine) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([c.size for c in mine])
        torch.cuda.synchronize()
        counts = runner.run_round(buf, offs)
        # (a round of several targets may end on a batch of its own making — stopped targets matched again — so its rows are
        # taken per contig only in rounds of one; the counts of every round are compared either way)
        rows = [np.asarray(h.batch_matches(0, int(counts[0])))] if round_size == 1 else [np.asarray(counts, dtype=np.uint64)]
        grown = []
        for k in sorted(runner.streams):
            grown.append(digest(np.frombuffer(bytes(runner.streams[k][seen[k]:]), dtype=np.uint8)))
            seen[k] = len(runner.streams[k])
        recs.append((tuple(digest(x) for x in rows), tuple(grown), digest(h.ht())))
        laps += h.loading_position() < last_pos
        last_pos = h.loading_position()
        if shift:
            uni, n = check_invariant(h, "shift %d, round %d" % (shift, r))
            share = uni / n
    runner.flush()
    out = dict(recs=recs, streams={k: bytes(v) for k, v in runner.streams.items()}, locks=bytes(runner.locks_stream),
               ext=bytes(runner.ref_ext_sizes), ht=h.ht(), laps=laps, share=share, applied=tuple(runner.spec_local[:2]))
    h.close()
    return out


def test_the_summary_off_equals_the_oracle_loop():
    gs = collection()
    a = rounds_run(0)
    o = _orc.OracleMatcher(LIM)
    res = _driver.encode_rounds(o, lambda: _orc.OracleEmitter(o), [gs[0]], [[g] for g in gs[1:]], 1)
    for k, v in res["streams"].items():
        assert a["streams"][k] == v, k
    assert a["locks"] == res["locks"] and a["ext"] == res["refExtSize"]
    assert np.array_equal(a["ht"], o.ht())
    assert o.loaded_ref_length() > 3 * LIM and a["laps"] >= 3
    o.close()


@pytest.mark.parametrize("shift", SHIFTS[1:])
def test_rounds_are_the_same_at_every_shift(shift):
    a, b = rounds_run(0), rounds_run(shift)
    assert len(a["recs"]) == len(b["recs"]) == N_GENOMES - 1
    for r, (x, y) in enumerate(zip(a["recs"], b["recs"])):
        assert x[0] == y[0], "round %d: match rows differ at shift %d" % (r, shift)
        assert x[1] == y[1], "round %d: streams differ at shift %d" % (r, shift)
        assert x[2] == y[2], "round %d: table image differs at shift %d" % (r, shift)
    for k in a["streams"]:
        assert a["streams"][k] == b["streams"][k], k
    assert a["locks"] == b["locks"] and a["ext"] == b["ext"] and np.array_equal(a["ht"], b["ht"])
    assert b["laps"] >= 3 and a["applied"] == b["applied"]


def test_most_blocks_are_uniform_at_16_slots_per_block():
    """(the invariant itself is asserted after every round inside rounds_run)"""
    b = rounds_run(4)
    print("shift 4: %.3f of the blocks uniform after %d laps; speculative finalizes tried / applied %r" % (b["share"], b["laps"], b["applied"]))
    assert b["share"] >= UNIFORM_SHARE


def test_rounds_of_several_targets():
    """four targets per round: a flush with several pieces, the lock window clipping most extensions"""
    a, b = rounds_run(0, 4), rounds_run(4, 4)
    assert a["recs"] == b["recs"] and a["streams"] == b["streams"] and np.array_equal(a["ht"], b["ht"])


# ---- the sequential paths, through the plain calls (load_ref and load_separator launch their kernels themselves)
@functools.lru_cache(maxsize=None)
def plain_run(shift, chains, L):
    base = synth.base_codes(60_000, 5)
    gs = [synth.genome(base, i, 0.02) for i in range(40)]
    h = make(700_000, shift, chains=chains, **({"L": L} if L else {}))
    h.disable_sliding_window()
    h.load_ref(gs[0], load_rc=True)
    out, laps, last = [], 0, h.loading_position()
    for i, g in enumerate(gs[1:]):
        out.append(digest(h.match(g, L or 32)))
        h.load_ref(g)
        h.load_separator(0)
        laps += h.loading_position() < last
        last = h.loading_position()
        if shift:
            check_invariant(h, "plain calls, shift %d, target %d" % (shift, i))
    out.append(digest(h.ht()))
    uni = check_invariant(h, "plain calls, end")[0] if shift else 0
    h.close()
    return out, laps, uni


@pytest.mark.parametrize("chains,L", [("1", None), (None, 64)], ids=["one_chain_per_wave", "K_above_the_four_chain_limit"])
@pytest.mark.parametrize("shift", [4, 12])
def test_sequential_paths(chains, L, shift):
    a, b = plain_run(0, chains, L), plain_run(shift, chains, L)
    assert a[0] == b[0]
    assert b[1] >= 3
    assert shift != 4 or b[2] > 0


# ---- a speculative finalize that is taken back
def wrapped_and_mispredicted():
    S = _spec.scenarios()
    k = S["k_wrap_crosses_the_end"]
    rnd = k.rounds[0]
    pred = [1, 1, 0, 1, 1]
    return _spec.Scenario("wrap_mispredicted", k.ref, [_spec.Round(rnd.contigs, pred)], [False], max_ref=k.max_ref, sw_factor=k.sw_factor)


SPEC_NAMES = ["a_all_extend", "b_none_extends", "c_mispredicted_3", "f_mixed", "f_rc_not_predicted", "g_given_up", "h_veto", "i_another_replica_said_no",
              "i_word_left_alone", "j_two_in_flight", "k_wrap_crosses_the_end", "k_wrap_stops_at_the_end", "wrap_mispredicted"]


@pytest.mark.parametrize("name", SPEC_NAMES)
def test_a_speculative_finalize_leaves_the_summary_of_the_plain_one(name):
    from mbgc_amd import binding
    scn = wrapped_and_mispredicted() if name == "wrap_mispredicted" else _spec.scenarios()[name]
    dev = _spec.DeviceBackend(binding)
    with environment(SWSEM_TAGSUM_SHIFT=4):
        A = _spec.run_path(dev, scn)
        B = _spec.run_path(dev, scn, [r.decision for r in A.rounds])
    branches = _spec.check(scn, A, B)
    if scn.want[0] is not None:
        assert [b == "applied" for b in branches] == scn.want
    for p in (A, B):
        p.m.emit_batch_end()
        uni, n = check_invariant(p.m, name)
        assert uni > 0
    sa, sb = A.m.tag_summary(), B.m.tag_summary()
    assert sa[1] == sb[1] == 4 and np.array_equal(sa[0], sb[0]), "%s (%s): %d summary entries differ" % (name, branches, int((sa[0] != sb[0]).sum()))
    assert np.array_equal(A.m.tags(), B.m.tags())
    print("%s: %s; %d of %d blocks uniform" % (name, ", ".join(branches), uni, n))
    _spec.close(A, B)
