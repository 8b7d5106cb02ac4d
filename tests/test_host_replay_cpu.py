"""The host half of every entry point under host sanitizers, without a GPU: md::Args, the size checks, the scratch carve and pool, the
LDS-attribute cache and the grid arithmetic in front of each launch (include/minddet_hip.h "Conventions": the checks complete before
any device or runtime call; size limits return 4).

tests/host/Makefile compiles minddet_amd/csrc/*.hip with ASan + UBSan on the host side and links them with a replay program and a
stand-in for the HIP runtime that keeps a ledger of every runtime call (no real runtime is linked: the program cannot open a device).
This module writes the calls -- every valid row of every tests/abi_cases*.py table, every single-defect call tests/abi_derive.py
derives from them (the calls tests/test_abi_checks_cpu.py makes in-process), and every row with hostile extents substituted -- into a
case file, replays it once, and holds the return codes and the ledger to the header's rules.  Nothing built with a sanitizer is loaded into python."""
import copy
import functools
import os
import re
import subprocess


from minddet_amd import _lib
from tests import abi_derive as ad
from tests.abi_cases import F, U8, T
from tests.test_workspace_cpu import BOUNDS, COVERED, DIMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
BUILD = os.path.join(HOST, "build")
I64_MAX = 2 ** 63 - 1
REPORT = re.compile(r"runtime error:|AddressSanitizer|ThreadSanitizer|LeakSanitizer|UndefinedBehaviorSanitizer")


def _pixels(o):
    return o[0].shape[0] * o[0].shape[1] * o[0].shape[2]


# entry point -> (the op whose md_<op>_workspace_bytes it is held to, the extents that function takes): tests/test_workspace_cpu.py's
# table and the training ops whose functions their own headers declare
WS_OP = dict(COVERED, md_conv_bwd_weight="md_conv_bwd_weight", md_conv1x1_bwd_weight="md_conv1x1_bwd_weight",
             md_conv2d_grouped_bwd_weight="md_conv2d_grouped_bwd_weight", md_grad_sumsq="md_grad_sumsq")
WS_DIMS = dict(DIMS,
               md_conv_bwd_weight=lambda o, at: (_pixels(o), at.cin, at.cout, at.kernel),
               md_conv1x1_bwd_weight=lambda o, at: (_pixels(o), at.cin, at.cout),
               md_conv2d_grouped_bwd_weight=lambda o, at: (_pixels(o), at.groups, at.k),
               md_grad_sumsq=lambda o, at: (o[0].shape[0],))

# hostile substitutions that turned out to be legal calls: id -> reason.  Only a case that differs from a valid row in a workspace
# extent may stand here (the derivation leaves workspace operands alone, so none does)
LEGAL_HOSTILE = {}

# No table row is a call without work, so such calls are derived (include/minddet_hip.h: "a call without work (an empty batch) returns 0
# whatever the pointers are"): row id -> the extent value that is the row's batch (images, samples, lists, anchors or boxes; it
# occurs nowhere else in the row).  It is replaced by 0 and the data pointer of every operand that is empty then by NULL ("the data
# pointer of every non-empty required operand must be non-NULL"); the call returns 0 and launches nothing.
EMPTY_BATCH = {"md_conv2d": 1, "md_conv1x1_dual": 1, "md_bottleneck": 1, "md_c3_pair": 1, "md_conv2d_grouped": 1, "md_stem_pool": 1,
               "md_stem_conv": 1, "md_sppf_pool": 1, "md_upsample_add": 1, "md_maxpool2d": 1, "md_pw_chain": 1, "md_standup_boxes": 4,
               "md_cn_assign_targets[pool]": 1}


@functools.lru_cache(maxsize=None)
def programs():
    """build/replay and build/replay_tsan, built by tests/host/Makefile (at most 16 jobs)"""
    jobs = max(1, min(16, len(os.sched_getaffinity(0))))
    r = subprocess.run(["make", "-C", HOST, f"-j{jobs}", "all"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return os.path.join(BUILD, "replay"), os.path.join(BUILD, "replay_tsan")


def run_program(argv):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=0")
    r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    return r.returncode, r.stdout, r.stderr


def replay(name, lines, max_reports=400):
    """-> ({id: (rc, [ledger words])}, [(id, sanitizer report)]).  A report ends the program (UBSan is fatal by the build flag); the
    replay is then resumed behind the command that died, so that one run names every finding."""
    exe, _ = programs()
    path = os.path.join(BUILD, f"cases_{name}.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    results, reports, first = {}, [], 0
    while first < len(lines) and len(reports) <= max_reports:
        code, out, err = run_program([exe, "cases", path, str(first)])
        last = None
        for ln in out.splitlines():
            w = ln.split(" ")
            if w[0] == "B":
                last = (int(w[1]), w[2])
            elif w[0] == "R":
                assert w[1] not in results, f"two commands named {w[1]}"
                results[w[1]] = (int(w[2]), w[3:])
        if code == 0 and out.rstrip().endswith("END") and not REPORT.search(err):
            break
        assert last is not None, (code, err[-2000:])
        reports.append((last[1], err.strip()[:1500] or f"exit code {code}"))
        first = last[0] + 1
    return results, reports


def with_workspace(case, nbytes):
    """the row with its workspace operand described as nbytes (absent optional operands in front of it stay NULL)"""
    c = copy.copy(case)
    at = max(case.nparam) - 1
    ops = list(case.operands[:at])
    ops += [T((1,), F, "opt", null=True) for _ in range(at - len(ops))]
    c.operands = ops + [T((nbytes,), U8, "opt", "free")]
    return ad.Call(c)


def without_workspace(case):
    c = copy.copy(case)
    c.operands = list(case.operands[:ad.workspace_index(case)])
    return ad.Call(c)


def ws_dims(case, shapes=None):
    """the extents the row's md_<op>_workspace_bytes takes, from the row's shapes or from substituted ones"""
    ops = case.operands
    if shapes is not None:
        ops = [copy.copy(t) for t in ops]
        for t, s in zip(ops, shapes):
            t.shape = tuple(s)
    return tuple(int(v) for v in WS_DIMS[WS_OP[case.sym]](ops, case.extra))


def ws_line(ident, op, dims):
    return " ".join(["WS", ident.replace(" ", "_"), op + "_workspace_bytes", str(len(dims))] + [str(v) for v in dims])


def fits(dims):
    return all(-2 ** 63 <= v <= I64_MAX for v in dims)


@functools.lru_cache(maxsize=None)
def written():
    """-> (lines, {id: what the line is}) of the main replay"""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lines, meta = [], {}

    def add(ident, line, **kw):
        ident = ident.replace(" ", "_")
        assert ident not in meta, ident
        meta[ident] = kw
        lines.append(line)

    for table, case in ad.all_rows():
        base = f"{table}/{case.id}"
        ws = ad.workspace_index(case)
        valid_dims = ws_dims(case) if case.sym in WS_OP else None
        # every valid row: as written; without its workspace (the pool); with a workspace of exactly the library's answer; one byte short
        add(f"valid/{base}/row", ad.call_line(f"valid/{base}/row", ad.Call(case)), kind="valid", case=case)
        if ws is not None:
            add(f"valid/{base}/pool", ad.call_line(f"valid/{base}/pool", without_workspace(case)), kind="valid", case=case)
        if valid_dims is not None:
            need = _lib.workspace_bytes(WS_OP[case.sym], *valid_dims)
            add(f"wsfn/{base}/valid", ws_line(f"wsfn/{base}/valid", WS_OP[case.sym], valid_dims), kind="wsfn_valid", want=need)
            add(f"valid/{base}/exact", ad.call_line(f"valid/{base}/exact", with_workspace(case, need)), kind="valid", case=case)
            if need > 16:       # (Scratch::acquire holds an answer of 0 to 16 bytes, tests/test_workspace_cpu.py)
                add(f"short/{base}", ad.call_line(f"short/{base}", with_workspace(case, need - 1)), kind="short")
        if case.id in EMPTY_BATCH:
            ec = ad.substituted(case, {EMPTY_BATCH[case.id]: 0})
            ec.null_ptr = [null or 0 in shape for null, shape in zip(ec.null_ptr, ec.shapes)]
            add(f"empty/{base}", ad.call_line(f"empty/{base}", ec), kind="empty")
        for k, (kind, i, call, want) in enumerate(ad.mutations(case)):
            add(f"defect/{base}/{k}:{kind}/{i}", ad.call_line(f"defect/{base}/{k}:{kind}/{i}", call), kind="defect", want=want)
        for label, table_, probe in ad.hostile_tables(case):
            call = ad.substituted(case, table_)
            # a probe (tests/abi_derive.py: every extent below the cap of Args::tensor, by membership in the PROBE sets) reaches the op's
            # own arithmetic, and a huge call may be legal; every other substitution is hostile and must be refused
            add(f"hostile/{base}/{label}", ad.call_line(f"hostile/{base}/{label}", call), kind="probe" if probe else "hostile")
            if valid_dims is not None:
                dims = ws_dims(case, call.shapes)
                if dims != valid_dims and fits(dims):
                    add(f"wsfn/{base}/{label}", ws_line(f"wsfn/{base}/{label}", WS_OP[case.sym], dims), kind="wsfn", dims=dims,
                        valid_dims=valid_dims, op=WS_OP[case.sym])
    return lines, meta


@functools.lru_cache(maxsize=None)
def replayed():
    lines, meta = written()
    results, reports = replay("abi", lines)
    return meta, results, reports


def launches(words):
    """[(kernel, grid, block, lds)] of a ledger"""
    out = []
    for w in words:
        if w.startswith("launch:"):
            _, name, grid, block, lds, _ = w.split(":")
            out.append((name, tuple(int(v) for v in grid.split(",")), tuple(int(v) for v in block.split(",")), int(lds)))
    return out


def illegal_launches(words, raised):
    """the launches of a ledger that the device would refuse or that lack their LDS attribute.  raised: kernel -> the largest
    attribute value set so far in the replay (the library caches it per kernel for the life of the process, so an earlier call's
    attribute call counts; the caller hands every ledger over in replay order)"""
    bad = []
    for w in words:
        if w.startswith("attr:"):
            _, name, _, value = w.split(":")
            raised[name] = max(raised.get(name, 0), int(value))
        elif w.startswith("launch:"):
            (name, grid, block, lds), = launches([w])
            vol = block[0] * block[1] * block[2]
            ok = min(grid) >= 1 and grid[0] <= 2 ** 31 - 1 and grid[1] <= 65535 and grid[2] <= 65535 and min(block) >= 1 and vol <= 1024
            ok = ok and lds <= 160 * 1024 and (lds <= 64 * 1024 or raised.get(name, 0) >= lds)
            if not ok:
                bad.append(w)
    return bad


def test_no_sanitizer_report_and_every_written_case_ran():
    meta, results, reports = replayed()
    assert not reports, f"{len(reports)} sanitizer reports, the first of them:\n" + "\n\n".join(f"{i}\n{r}" for i, r in reports[:5])
    assert set(results) == set(meta) and len(results) == len(written()[0])


def test_a_refused_call_has_touched_nothing():
    """every single-defect call returns its documented code, every hostile call 1, 2 or 4, a workspace one byte short 4 -- and the
    ledger of each is empty: no hipGetDevice, no allocation, no attribute call, no launch"""
    meta, results, _ = replayed()
    bad, legal = [], []
    for ident, m in meta.items():
        if m["kind"] not in ("defect", "hostile", "short") or ident not in results:
            continue
        rc, words = results[ident]
        if m["kind"] == "hostile" and rc == 0 and ident in LEGAL_HOSTILE:
            legal.append(ident)
            continue
        want = {"defect": (m.get("want"),), "short": (4,), "hostile": (1, 2, 4)}[m["kind"]]
        if rc not in want or words:
            bad.append((ident, rc, words[:4]))
    assert not bad, f"{len(bad)} refused calls with a wrong code or a runtime call (id, rc, ledger): {bad[:20]}"
    assert sorted(legal) == sorted(LEGAL_HOSTILE)
    assert all("workspace" in reason for reason in LEGAL_HOSTILE.values())
    kinds = [m["kind"] for m in meta.values()]
    assert kinds.count("defect") > 2000 and kinds.count("hostile") > 5000 and kinds.count("short") >= 20, \
        (kinds.count("defect"), kinds.count("hostile"), kinds.count("short"))


def test_a_valid_row_returns_0_and_launches_legally():
    meta, results, _ = replayed()
    bad, total, raised = [], 0, {}
    for ident, m in meta.items():
        if ident not in results:
            continue
        rc, words = results[ident]
        illegal = illegal_launches(words, raised)
        if m["kind"] == "empty" and (rc != 0 or [w for w in words if w != "lasterror"]):
            bad.append((ident, "a call without work must return 0 and neither allocate nor launch", rc, words[:4]))
        if m["kind"] != "valid":
            continue
        got = launches(words)
        total += len(got)
        if rc != 0:
            bad.append((ident, "rc", rc))
        if not got:
            bad.append((ident, "no launch", words[:4]))
        bad += [(ident, "illegal launch", w) for w in illegal]
    assert not bad, f"{len(bad)}: {bad[:20]}"
    assert total > 0, "the valid rows together recorded no launch: the ledger cannot see"
    assert {i.split("/", 2)[2] for i, m in meta.items() if m["kind"] == "empty"} == set(EMPTY_BATCH)


def test_extents_below_the_cap_are_refused_cleanly_or_run_as_legal_launches():
    """Rows whose extents are replaced by values that Args::tensor lets through (2^31 - 1; pairs and a triple whose product wraps
    `int`, or fits int64_t only until it is multiplied by an element width) reach the op's own size arithmetic.  Many ops set no
    limit on a tensor's size (their kernels stride over a size_t count), so such a call may be legal: it is then held to what a valid
    row is held to, rc 0 and legal launches only; otherwise it is refused with 2 or 4 and an empty ledger.  Either way no sanitizer
    report (the first test): the products are not allowed to wrap."""
    meta, results, _ = replayed()
    bad, n, accepted, raised = [], 0, 0, {}
    for ident, m in meta.items():
        if ident not in results:
            continue
        rc, words = results[ident]
        illegal = illegal_launches(words, raised)
        if m["kind"] != "probe":
            continue
        n += 1
        if rc == 0:
            accepted += 1
            bad += [(ident, "illegal launch", w) for w in illegal]
        elif rc not in (1, 2, 4) or words:
            bad.append((ident, rc, words[:4]))
    assert not bad, f"{len(bad)}: {bad[:20]}"
    assert n > 2000 and 0 < accepted < n, (n, accepted)


def test_workspace_functions_refuse_what_does_not_fit():
    """-1 for a negative extent and for a byte count that does not fit int64_t; otherwise never below the valid row's answer when no
    extent is below the valid row's; equal to the header's formula where the header states one exactly"""
    meta, results, _ = replayed()
    bad, n = [], 0
    for ident, m in meta.items():
        if ident not in results:
            continue
        got = results[ident][0]
        if m["kind"] == "wsfn_valid":
            if got != m["want"]:
                bad.append((ident, got, m["want"]))
        elif m["kind"] == "wsfn":
            n += 1
            dims, op = m["dims"], m["op"]
            valid = results["wsfn/" + ident.split("/", 1)[1].rsplit("/", 1)[0] + "/valid"][0]
            if min(dims) < 0:
                ok = got == -1
            else:
                ok = got == -1 or got >= 0
                if all(a >= b for a, b in zip(dims, m["valid_dims"])):
                    ok = ok and (got == -1 or got >= valid)
                if op in BOUNDS:
                    cap = BOUNDS[op][1](*dims)
                    if BOUNDS[op][2]:
                        ok = ok and got == (cap if cap <= I64_MAX else -1)
                    elif got != -1:
                        ok = ok and got <= cap
            if not ok:
                bad.append((ident, dims, got))
    assert not bad, f"{len(bad)}: {bad[:20]}"
    assert n > 500, n


# ----- the scratch pool (csrc/aot.h): one buffer per (device, stream), 64 of them, grown on demand; md_scratch_release frees all
def _pool_row():
    from tests import abi_cases_cn
    return next(c for c in abi_cases_cn.CASES if c.id == "md_cn_assign_targets[pool]")


def _events(words, name):
    return [w.split(":") for w in words if w.startswith(name + ":")]


def test_the_scratch_pool_keeps_one_buffer_per_stream_and_frees_what_it_took():
    row = _pool_row()
    small = ad.Call(row)                                      # 16 B M = 64 bytes of scratch
    large = ad.Call(row)                                      # B = 1024, M = 128: 2 MiB
    large.shapes = [[1024, 3, 4], [1024, 3], [1024, 3, 8, 12], [1024, 128], [1024, 128], [1024, 128, 2], [1024, 128, 2]]
    need_large = _lib.workspace_bytes("md_cn_assign_targets", 1024, 128)
    assert need_large == 2 << 20
    stream = lambda k: 0x1000 * (k + 1)
    lines = [ad.call_line(f"first/{k}", small, stream(k)) for k in range(70)]
    lines += [ad.call_line(f"again/{k}", small, stream(k)) for k in (0, 63, 64)]
    lines += [ad.call_line("grow/5", large, stream(5)), ad.call_line("shrink/5", small, stream(5)), ad.call_line("large_again/5", large, stream(5))]
    lines += ["RELEASE release", "BALANCE balance"]
    lines += ["FAILALLOC fail 2", ad.call_line("failed", small, stream(99)), "BALANCE balance_after_failure", "RELEASE release2",
              "BALANCE balance_end"]
    results, reports = replay("pool", lines)
    assert not reports, reports[:3]
    for k in range(70):
        rc, words = results[f"first/{k}"]
        mallocs, frees = _events(words, "malloc"), _events(words, "freeasync")
        assert rc == 0 and len(mallocs) == 1 and int(mallocs[0][2], 16) == stream(k), (k, rc, words)
        if k < 64:      # pooled: 1 MiB, the pool's first step, and it stays
            assert int(mallocs[0][1]) == 1 << 20 and not frees, (k, words)
        else:           # the pool is full: a one-call allocation of what the op takes, freed on the stream within the call
            assert int(mallocs[0][1]) == 64 and len(frees) == 1 and int(frees[0][1]) == 64 and int(frees[0][2], 16) == stream(k), (k, words)
    for k in (0, 63):
        assert not _events(results[f"again/{k}"][1], "malloc"), k
    assert len(_events(results["again/64"][1], "malloc")) == len(_events(results["again/64"][1], "freeasync")) == 1
    rc, words = results["grow/5"]
    assert rc == 0 and [int(m[1]) for m in _events(words, "malloc")] == [2 << 20], words
    assert [(int(f[1]), int(f[2], 16)) for f in _events(words, "freeasync")] == [(1 << 20, stream(5))], words
    for ident in ("shrink/5", "large_again/5"):
        assert results[ident][0] == 0 and not _events(results[ident][1], "malloc") and not _events(results[ident][1], "freeasync"), ident
    rc, words = results["release"]
    assert rc == 0 and sorted(int(f[1]) for f in _events(words, "free")) == [1 << 20] * 63 + [2 << 20], words
    live, words = results["balance"]
    assert live == 0 and words[0].split(":")[1] == words[1].split(":")[1], words           # allocations == frees: nothing leaked
    # an allocation that fails (the pool's and the one-call fallback's): rc 3, nothing launched, nothing left behind
    rc, words = results["failed"]
    assert rc == 3 and words.count("malloc_failed") == 2 and not launches(words) and not _events(words, "malloc"), words
    assert results["balance_after_failure"][0] == 0 and results["release2"][0] == 0 and results["balance_end"][0] == 0


def test_the_lds_attribute_cache_sets_once_per_kernel_and_size_increase():
    exe, _ = programs()
    code, out, err = run_program([exe, "lds"])
    assert code == 0 and out.rstrip().endswith("END") and not REPORT.search(err), err[-2000:]
    sets = {}
    for ln in out.splitlines():
        w = ln.split(" ")
        if w[0] == "L":
            assert int(w[3]) == 0, ln                               # MD_OK, also for the kernels the full table has no slot for
            sets[int(w[1]), int(w[2])] = [x for x in w[4:] if x.startswith("attr:")]
    assert len(sets) == 4 * 130
    values = lambda step: [[int(a.split(":")[3]) for a in sets[step, i]] for i in range(130)]
    assert values(0) == [[70000]] * 130 and values(2) == [[90000]] * 130
    uncached = [i for i in range(130) if sets[1, i]]
    assert len(uncached) == 2 and values(1) == [[70000] if i in uncached else [] for i in range(130)]
    assert values(3) == [[80000] if i in uncached else [] for i in range(130)]


def test_pool_and_lds_cache_under_eight_threads_without_a_race_report():
    _, exe = programs()
    code, out, err = run_program([exe, "threads"])
    assert code == 0 and not REPORT.search(err) and not REPORT.search(out), err[-3000:]
    t = next(ln for ln in out.splitlines() if ln.startswith("T ")).split(" ")
    assert t[1:3] == ["0", "0"] and t[3].split(":")[1] == t[4].split(":")[1] and t[5] == "live:0", out
