"""The dynamic LDS layouts of the launched kernels (squarna_amd/csrc/sq_launch_lds.h), compiled for the host with a plain C++
compiler.  tests/native/launch_lds_host.cpp prints a layout per input line as JSON; this file states every size a second time --
the formulas the launch sites held before the layouts had one place -- and checks what a carving must have: aligned regions that
do not overlap and end inside the total, a shorter job's regions inside the room of the launch's longest, and every decision on
both sides of its threshold.  The same harness is built a second time as a stand-alone program with the address and
undefined-behaviour sanitizers and run on the same input."""
import itertools
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "launch_lds_host.cpp")
BUILD = os.path.join(HERE, "native", "_build")

NS = [1, 4, 5, 15, 16, 17, 31, 32, 33, 200, 201, 4095, 4096, 4097, 8000, 8001, 16384, 16385]
LETTERS = [1, 4, 29]
THREADS = [64, 128, 256, 512, 1024]
CELLS = [25, 1056]
STR_CAPS = [0, 4, 1024]
NSURV = [64, 384, 1024]
BITWORDS = [2, 128, 129, 1024]
WIDTHS = [(4, 256), (16, 1024)]                      # (waves, keycap) of the ranking kernel's two block widths
TMAX = [1, 8, 100, 11264]
NR_LIM, STATE_LIM = 4096, 24 * 1024                  # the defaults of SQ_SCORE_NR_LIM / SQ_SCORE_STATE_LIM
#: the mode-0 launch of float-reactivity records (512 threads, 1,024 strands, cell table of 32) asks for more than 64 KB from 1,277 nt
#: on, for no more than 64 KB again from 1,635 nt (the state copies no longer fit SQ_SCORE_STATE_LIM and leave), and for more from
#: 2,125 nt on for good; tests/test_hip_launch_lds.py folds records of the first and the last length
SCORE_CROSSINGS = [1277, 1635, 2125]


def _build(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("launch_lds_host", ["-O2"])


@pytest.fixture(scope="module")
def exe_san():
    return _build("launch_lds_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, cmd, rows):
    res = subprocess.run([exe, cmd], input="".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = [json.loads(x) for x in res.stdout.strip().split("\n")] if res.stdout.strip() else []
    assert len(out) == len(rows), (cmd, len(out), len(rows))
    return out


def constants(exe):
    res = subprocess.run([exe, "constants"], capture_output=True, text=True, check=True)
    return json.loads(res.stdout)


def regions(row):
    return {k: v for k, v in row.items() if isinstance(v, list)}


def check_carve(row, what, wide=()):
    """every region on a multiple of its element size (`wide`: of 16 bytes), no two overlapping, each ending inside the total"""
    regs = [(off, off + size * count, k, size) for k, (off, size, count) in regions(row).items() if count]
    for lo, hi, k, size in regs:
        assert lo % (16 if k in wide else size) == 0, (what, k)
        assert hi <= row["total"], (what, k)
    regs.sort()
    for (_, hi, k, _), (lo, _, k2, _) in zip(regs, regs[1:]):
        assert hi <= lo, (what, k, k2)


# ---- the formulas of the launch sites before sq_launch_lds.h ----------------------------------------------------------------------

def fill_bytes(n):
    return 12 * ((n + 15) & ~15) + 64


def masks_bytes(n, letters):
    nw = (n + 31) // 32
    return 3 * ((n + 3) & ~3) + 4 * letters * (nw + 3) + 4 * nw * letters + 16


def state_bytes(maxn):
    lds_n = maxn if maxn <= 8000 else 0
    return 7 * ((lds_n + 8) & ~7) + 64 if lds_n else 0


def score_ints(lds_n, lds_nr, lds_ns, cell_entries, thr, mode, str_cap):
    """(cell_off, surv_off, str_off, dyn) as sq_launch_round_kernels added them up"""
    dyn = ((lds_n + 15) & ~15) + 8 * lds_nr + 6 * ((lds_ns + 8) & ~7) + 16 if lds_n else 0
    cell_off = (dyn + 15) & ~15
    dyn = cell_off + 8 * cell_entries
    surv_off = (dyn + 15) & ~15
    dyn = surv_off + 14 * (4 + (1 if mode == 0 else 0)) * thr
    str_off = (dyn + 15) & ~15
    if mode == 0:
        dyn = str_off + 10 * str_cap + 16
    return cell_off, surv_off, str_off, dyn


def score_decisions(maxn, need_reacts, mode, nr_lim, state_lim):
    lds_n = maxn if maxn <= 16384 else 0
    lds_nr = maxn if need_reacts and maxn <= nr_lim else 0
    dyn_base = ((lds_n + 15) & ~15) + 8 * lds_nr + 16 if lds_n else 0
    lds_ns = maxn if lds_n and mode == 0 and dyn_base + 6 * ((maxn + 8) & ~7) <= state_lim else 0
    return lds_n, lds_nr, lds_ns


def rank_bytes(thr, bitwords, keycap):
    refp_lds = bitwords <= 128
    return ((((thr // 64) * bitwords + 1) & ~1) * 4) + keycap * 24 + ((keycap + 7) & ~7) + 32 * bitwords + 16 + (64 * bitwords if refp_lds else 0)


def extend_bytes(T):
    return ((T + 7) & ~7) * 14 + 64 * 4 + 64


def pack_bytes(maxn, tmax):
    rowcap = (maxn + 8) & ~7
    return ((rowcap * 2 + 15) & ~15) + extend_bytes(tmax)


def pairs_bytes(maxn):
    return ((maxn + 3) & ~3) * 4 + 16


def score_rows():
    rows = []
    for n in NS:
        lds_n = n if n <= 16384 else 0
        for nr, ns, thr, mode, cell, cap in itertools.product((0, lds_n), (0, lds_n), THREADS, (0, 1), CELLS, STR_CAPS):
            rows.append((lds_n, nr, ns, cell, thr, mode, cap, n if lds_n else 0))
    return rows


def all_inputs():
    return [("fill", [(n,) for n in NS]), ("masks", [(n, l) for n in NS for l in LETTERS]), ("state", [(n,) for n in NS]),
            ("scan", [(n, fb) for n in NS if n <= 200 for fb in (64, 128, 2048)]), ("score", score_rows()),
            ("choose", [(n,) for n in NSURV]), ("rank", [(w, bw, kc) for w, kc in WIDTHS for bw in BITWORDS]),
            ("pack", [(n, t) for n in NS for t in TMAX]), ("pairs", [(n,) for n in NS]), ("crossing", [(32,)])]


def test_constants_once_each(exe):
    assert constants(exe) == dict(plain_max=64 * 1024, block_max=160 * 1024, fill_n=4096, masks_max=60 * 1024, state_n=8000,
                                  score_n=16384, refp_words=128, chunk=4, strands=1024)


def test_totals_equal_the_formulas_of_the_launch_sites(exe):
    for (n,), r in zip([(n,) for n in NS], run(exe, "fill", [(n,) for n in NS])):
        assert r["total"] == fill_bytes(n), n
    rows = [(n, l) for n in NS for l in LETTERS]
    for (n, l), r in zip(rows, run(exe, "masks", rows)):
        assert r["total"] == masks_bytes(n, l) and r["nw"] == r["bits_nw"] == (n + 31) // 32, (n, l)
    for n, r in zip(NS, run(exe, "state", [(n,) for n in NS])):
        assert r["total"] == state_bytes(n), n
    rows = [(n, fb) for n in NS if n <= 200 for fb in (64, 128, 2048)]
    for (n, fb), r in zip(rows, run(exe, "scan", rows)):
        assert r["scan"] == r["scan6"] == 4 * fb and r["state"] == 7 * ((n + 8) & ~7) + 64 and r["total"] == max(r["state"], 4 * fb), (n, fb)
    rows = score_rows()
    assert len(rows) == len(NS) * 2 * 2 * 5 * 2 * 2 * 3
    for row, r in zip(rows, run(exe, "score", rows)):
        cell_off, surv_off, str_off, dyn = score_ints(*row[:7])
        assert (r["cell"][0], r["surv_bps"][0], r["total"]) == (cell_off, surv_off, dyn), row
        if row[5] == 0:
            assert r["str"][0] == str_off and r["str"][2] == r["skip"][2] == row[6], row
        thr, per = row[4], 5 if row[5] == 0 else 4
        assert r["surv_bps"][2] == r["surv_key"][2] == r["surv_len"][2] == per * thr
        assert r["surv_len"][0] + 2 * per * thr - surv_off == 14 * per * thr and r["skip"][0] + 2 * r["skip"][2] - r["str"][0] == 10 * r["str"][2]
    for n, r in zip(NSURV, run(exe, "choose", [(n,) for n in NSURV])):
        assert r["total"] == 18 * n + 16, n
    rows = [(w, bw, kc) for w, kc in WIDTHS for bw in BITWORDS]
    for (w, bw, kc), r in zip(rows, run(exe, "rank", rows)):
        assert r["total"] == rank_bytes(64 * w, bw, kc) and r["refp_lds"] == (bw <= 128), (w, bw)
        assert r["pri"][0] - r["key"][0] == 24 * kc and r["pri"][1] * r["pri"][2] == kc          # 24 + 1 bytes per key
    rows = [(n, t) for n in NS for t in TMAX]
    for (n, t), r in zip(rows, run(exe, "pack", rows)):
        assert r["total"] == pack_bytes(n, t) and r["ext_bytes"] == extend_bytes(t) and r["rowcap"] == (n + 8) & ~7, (n, t)
        assert r["ext_of_rowcap"] == r["ext"][0]                                   # (the kernel places the scratch from its rowcap)
    for n, r in zip(NS, run(exe, "pairs", [(n,) for n in NS])):
        assert r["total"] == pairs_bytes(n), n


def test_regions_are_aligned_disjoint_and_inside_the_total(exe):
    for cmd, rows in all_inputs():
        if cmd in ("scan", "crossing"):
            continue
        for row, r in zip(rows, run(exe, cmd, rows)):
            if cmd == "state" and not r["lds_n"]:
                continue                                                              # assembled in global memory: no LDS
            if cmd == "score":
                if not r["reacts_fit"] or not row[0]:                                 # (lds_n == 0: nothing is staged by length)
                    del r["reacts"]
                if not r["state_fits"] or not row[0]:
                    r.pop("P"), r.pop("U"), r.pop("SU")
            check_carve(r, (cmd, row), wide=("cell", "str", "ext"))
            if cmd == "state":
                assert r["carved"] == 1 and all(r[k][2] <= (r["U"][0] - r["P"][0]) // 2 for k in ("P", "U", "SU", "E")), row


def test_a_shorter_job_lies_inside_the_room_of_the_longest(exe):
    """Whatever a block places by its own job's length must end inside what the launch asked for by its longest job (the fill
    once asked for nothing when the longest sequence was beyond its limit, and shorter jobs staged all the same)."""
    pairs = [(a, b) for b in NS for a in NS if a <= b]
    fill = dict(zip(NS, run(exe, "fill", [(n,) for n in NS])))
    for a, b in pairs:
        if a <= 4096 and b <= 4096:
            assert all(off + size * count <= fill[b]["total"] for off, size, count in regions(fill[a]).values()), (a, b)
    # (the launch sizes the fill by the longest job that may stage: a batch with a 4,097-nt job sizes it by the next longest)
    assert [fill[n]["staged"] for n in (4096, 4097)] == [1, 0]
    mrows = [(n, l) for n in NS for l in LETTERS]
    masks = dict(zip(mrows, run(exe, "masks", mrows)))
    for (a, b), l, l2 in itertools.product(pairs, LETTERS, LETTERS):
        if l2 <= l:                                  # the kernel carves by (job n, the launch's letters); fewer letters: smaller still
            for job in (masks[(a, l)], masks[(a, l2)]):
                assert all(off + size * count <= masks[(b, l)]["total"] for off, size, count in regions(job).values()), (a, b, l, l2)
    state = dict(zip(NS, run(exe, "state", [(n,) for n in NS])))
    for a, b in pairs:
        if b <= 8000:                                # carved by the launch's lds_n: a job fills a + 1 entries of sections of np
            np_b = (state[b]["U"][0] - state[b]["P"][0]) // 2
            assert a + 1 <= np_b and state[a]["total"] <= state[b]["total"], (a, b)
    rows = [(b, nr, ns, cell, 512, 0, 1024, a) for a, b in pairs if b <= 16384 for nr in (0, b) for ns in (0, b) for cell in CELLS]
    for row, r in zip(rows, run(exe, "score", rows)):
        a, b = row[7], row[0]
        assert r["ci_fits"] == 1 and r["reacts_fit"] == (row[1] >= a) and r["state_fits"] == (row[2] >= a), row
        if not r["reacts_fit"]:
            del r["reacts"]
        if not r["state_fits"]:
            r.pop("P"), r.pop("U"), r.pop("SU")
        check_carve(r, row, wide=("cell", "str"))    # the job's codes / reactivities below the launch's regions, all inside the total
        if r["state_fits"]:
            assert a + 1 <= r["state_np"]


def test_every_decision_on_both_sides_of_its_threshold(exe):
    fill = run(exe, "fill", [(4096,), (4097,)])
    assert [r["staged"] for r in fill] == [1, 0] and fill[0]["total"] <= 64 * 1024
    state = run(exe, "state", [(8000,), (8001,)])
    assert [r["lds_n"] for r in state] == [8000, 0] and [r["total"] for r in state] == [56120, 0]
    rows = [(n, need, mode, nr_lim, lim) for n in NS + [64, 65, 1634, 1635] for need in (0, 1) for mode in (0, 1)
            for nr_lim in (64, NR_LIM) for lim in (1, STATE_LIM, 1 << 20)]
    for row, r in zip(rows, run(exe, "decide", rows)):
        assert (r["lds_n"], r["lds_nr"], r["lds_ns"]) == score_decisions(*row), row
    dec = lambda *row: tuple(run(exe, "decide", [row])[0][k] for k in ("lds_n", "lds_nr", "lds_ns"))
    assert dec(16384, 0, 1, NR_LIM, STATE_LIM)[0] == 16384 and dec(16385, 0, 1, NR_LIM, STATE_LIM)[0] == 0
    assert dec(4096, 1, 0, NR_LIM, STATE_LIM)[1] == 4096 and dec(4097, 1, 0, NR_LIM, STATE_LIM)[1] == 0
    assert dec(64, 1, 0, 64, STATE_LIM)[1] == 64 and dec(65, 1, 0, 64, STATE_LIM)[1] == 0 and dec(64, 0, 0, 64, STATE_LIM)[1] == 0
    # state copies: (n up to 16) + 8 n + 16 + 6 (n + 1 up to 8) <= 24,576 holds up to 1,634 nt with reactivities staged, 3,503 without
    assert dec(1634, 1, 0, NR_LIM, STATE_LIM)[2] == 1634 and dec(1635, 1, 0, NR_LIM, STATE_LIM)[2] == 0
    assert dec(3503, 0, 0, NR_LIM, STATE_LIM)[2] == 3503 and dec(3504, 0, 0, NR_LIM, STATE_LIM)[2] == 0
    assert dec(200, 0, 0, NR_LIM, 1)[2] == 0 and dec(200, 0, 1, NR_LIM, STATE_LIM)[2] == 0
    for letters in (4, 29):
        n = max(k for k in range(1, 40000) if masks_bytes(k, letters) <= 60 * 1024)
        lo, hi = run(exe, "masks", [(n, letters), (n + 1, letters)])
        assert (lo["fit"], hi["fit"]) == (1, 0) and lo["total"] <= 60 * 1024 < hi["total"], (letters, n)
    assert [r["refp_lds"] for r in run(exe, "rank", [(4, 128, 256), (4, 129, 256)])] == [1, 0]
    lim = run(exe, "limits", [(64 * 1024,), (64 * 1024 + 1,), (160 * 1024,), (160 * 1024 + 1,)])
    assert [(r["raise"], r["fits"]) for r in lim] == [(0, 1), (1, 1), (1, 1), (1, 0)]
    # the launches that neither raise nor refuse stay below 64 KB by their own gates
    assert max(fill_bytes(4096), state_bytes(8000), 60 * 1024, 18 * 1024 + 16) <= 64 * 1024


def test_where_the_score_launch_crosses_64_kb(exe):
    """Float reactivities, mode 0, 512 threads, 1,024 strands, the smallest cell table a batch has (32 doubles): 15 n + 46,3xx
    bytes while the state copies are staged, 9 n + 46,4xx without them."""
    (r,) = run(exe, "crossing", [(32,)])
    assert [r[k] for k in sorted(r)] == SCORE_CROSSINGS
    for n, over in ((1276, False), (1277, True), (1634, True), (1635, False), (2124, False), (2125, True)):
        assert (score_ints(*score_decisions(n, True, 0, NR_LIM, STATE_LIM), 32, 512, 0, 1024)[3] > 64 * 1024) == over, n


def test_the_sanitized_harness_on_the_same_input(exe, exe_san):
    for cmd, rows in all_inputs():
        assert run(exe_san, cmd, rows) == run(exe, cmd, rows), cmd
    assert constants(exe_san) == constants(exe)
