"""The image plan of tf_fb_calc_slots (transflow_amd/csrc/fb_plan.h): which frame slots a call expands, in which runs,
and which two expansions every pair compares.  tools/fb_plan_host_check.cpp runs the header alone on the CPU, under the
sanitizers where they link, every buffer a heap block of exactly its capacity.  The expectations are the rules':

  share     the slots in first-seen order, one run {0, 0, n}
  no_share  one entry per pair and side, map (2i, 2i+1), one run {0, 0, 2 n_pairs}
  keep      the slots that are not expanded (or are external), sorted and cut into runs of consecutive slots
            {first slot, offset in the list, slots}; the map is the slot pairs themselves
  every run starts at an even offset and is padded to an even length with its first slot
  a list or a run that does not fit its capacity is an error, and nothing is written behind the capacity
"""
import os
import random
import subprocess

from tests.helpers import build_host_check

PREV, NEXT = [0, 1, 2, 3, 3, 1, 4, 2], [1, 2, 3, 4, 3, 0, 0, 3]


def _case(name, mode, slots, max_pairs, prev, nxt, expanded=None, external=None, list_cap=-1):
    fields = [name, mode, str(slots), str(max_pairs), str(list_cap),
              "prev=" + ",".join(map(str, prev)), "next=" + ",".join(map(str, nxt))]
    if expanded is not None:
        fields.append("expanded=" + ",".join(map(str, expanded)))
    if external is not None:
        fields.append("external=" + ",".join(map(str, external)))
    return " ".join(fields)


def _plan(tmp_path, lines):
    """name -> the program's lines for it ({"list": [..], "map": [..], "runs": [..]} or "error")"""
    program, sanitized = build_host_check(tmp_path, "fb_plan_host_check.cpp")
    print("sanitized" if sanitized else "not sanitized: the sanitizer runtime does not link here")
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([program, str(cases)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = {}
    for line in run.stdout.splitlines():
        name, what, *rest = line.split()
        if what == "error":
            got[name] = "error"
        else:
            got.setdefault(name, {})[what] = " ".join(rest)
    return got


# (the case line, what the rules give)
CASES = [
    (_case("share", "share", 5, 8, PREV, NEXT),
     {"list": "0 1 2 3 4 0", "map": "(0,1) (1,2) (2,3) (3,4) (3,3) (1,0) (4,0) (2,3)", "runs": "{0,0,5}"}),
    (_case("no_share", "no_share", 5, 8, PREV, NEXT),
     {"list": "0 1 1 2 2 3 3 4 3 3 1 0 4 0 2 3",
      "map": "(0,1) (2,3) (4,5) (6,7) (8,9) (10,11) (12,13) (14,15)", "runs": "{0,0,16}"}),
    (_case("no_share_exact_fit", "no_share", 5, 8, PREV, NEXT, list_cap=16),
     {"list": "0 1 1 2 2 3 3 4 3 3 1 0 4 0 2 3",
      "map": "(0,1) (2,3) (4,5) (6,7) (8,9) (10,11) (12,13) (14,15)", "runs": "{0,0,16}"}),
    (_case("no_share_short", "no_share", 5, 8, PREV, NEXT, list_cap=15), "error"),
    (_case("share_short", "share", 5, 8, PREV, NEXT, list_cap=5), "error"),  # the pad entry counts
    (_case("keep_two_runs", "keep", 6, 3, [1, 4, 0], [2, 5, 3], [1, 0, 0, 1, 0, 1], [0, 0, 0, 0, 0, 1]),
     {"list": "1 2 4 5", "map": "(1,2) (4,5) (0,3)", "runs": "{1,0,2} {4,2,2}"}),
    (_case("keep_odd_run", "keep", 4, 2, [1, 2], [2, 3], [1, 0, 0, 0]),
     {"list": "1 2 3 1", "map": "(1,2) (2,3)", "runs": "{1,0,3}"}),
    (_case("keep_singles", "keep", 3, 2, [0, 1], [1, 2], [0, 1, 0]),
     {"list": "0 0 2 2", "map": "(0,1) (1,2)", "runs": "{0,0,1} {2,2,1}"}),
    (_case("keep_nothing", "keep", 2, 1, [0], [1], [1, 1]),
     {"list": "", "map": "(0,1)", "runs": ""}),
    # slots = 2P, every other slot needed and the rest expanded, P pairs naming them all: P runs of one, 2P entries
    (_case("keep_worst", "keep", 8, 4, [0, 2, 4, 6], [1, 3, 5, 7], [0, 1, 0, 1, 0, 1, 0, 1]),
     {"list": "0 0 2 2 4 4 6 6", "map": "(0,1) (2,3) (4,5) (6,7)", "runs": "{0,0,1} {2,2,1} {4,4,1} {6,6,1}"}),
    (_case("keep_worst_exact_fit", "keep", 8, 4, [0, 2, 4, 6], [1, 3, 5, 7], [0, 1, 0, 1, 0, 1, 0, 1], list_cap=8),
     {"list": "0 0 2 2 4 4 6 6", "map": "(0,1) (2,3) (4,5) (6,7)", "runs": "{0,0,1} {2,2,1} {4,4,1} {6,6,1}"}),
    (_case("keep_worst_short", "keep", 8, 4, [0, 2, 4, 6], [1, 3, 5, 7], [0, 1, 0, 1, 0, 1, 0, 1], list_cap=7), "error"),
    # every slot of 2P needed: one run, no pad
    (_case("keep_all", "keep", 8, 4, [0, 2, 4, 6], [1, 3, 5, 7], [0] * 8),
     {"list": "0 1 2 3 4 5 6 7", "map": "(0,1) (2,3) (4,5) (6,7)", "runs": "{0,0,8}"}),
    # an expanded slot is listed again once it is external (written behind the library's back)
    (_case("keep_external", "keep", 2, 1, [0], [1], [1, 1], [0, 1]),
     {"list": "1 1", "map": "(0,1)", "runs": "{1,0,1}"}),
    (_case("same_slot_share", "share", 2, 1, [1], [1]), {"list": "1 1", "map": "(0,0)", "runs": "{0,0,1}"}),
    (_case("same_slot_no_share", "no_share", 2, 1, [1], [1]), {"list": "1 1", "map": "(0,1)", "runs": "{0,0,2}"}),
    (_case("same_slot_keep", "keep", 2, 1, [1], [1], [0, 0]), {"list": "1 1", "map": "(1,1)", "runs": "{1,0,1}"}),
]


def test_plan_cases(tmp_path):
    got = _plan(tmp_path, [line for line, _ in CASES])
    for line, want in CASES:
        name = line.split()[0]
        assert got.get(name) == want, (name, got.get(name), want)


def _model(mode, slots, prev, nxt, expanded, external):
    """The rules of the module docstring, restated: (list, map, runs)."""
    if mode == "keep":
        need = sorted({s for s in prev + nxt if not expanded[s] or external[s]})
        lst, runs = [], []
        while need:
            run = [need.pop(0)]
            while need and need[0] == run[-1] + 1:
                run.append(need.pop(0))
            runs.append((run[0], len(lst), len(run)))
            lst += run + ([run[0]] if len(run) % 2 else [])
        return lst, list(zip(prev, nxt)), runs
    lst, pairs = [], []
    for a, b in zip(prev, nxt):
        pair = []
        for s in (a, b):
            if mode == "no_share" or s not in lst:
                lst.append(s)
                pair.append(len(lst) - 1)
            else:
                pair.append(lst.index(s))
        pairs.append(tuple(pair))
    n = len(lst)
    return lst + ([lst[0]] if n % 2 else []), pairs, [(0, 0, n)]


def test_plan_sweep(tmp_path):
    """Random small handles in every mode against the restated rules; no list is longer than 4 P (what the handle's
    staging buffer holds), whatever the flags."""
    rng = random.Random(7)
    lines, want = [], {}
    for i in range(600):
        mode = ("share", "no_share", "keep")[i % 3]
        P = rng.randint(1, 4)
        slots = rng.randint(2, 2 * P if mode == "keep" else 9)  # tf_fb_keep_expansions: slots <= 2 P
        n = rng.randint(1, P)
        prev = [rng.randrange(slots) for _ in range(n)]
        nxt = [rng.randrange(slots) for _ in range(n)]
        expanded = [rng.randint(0, 1) for _ in range(slots)]
        external = [int(rng.random() < 0.2) for _ in range(slots)]
        name = f"sweep{i}"
        lines.append(_case(name, mode, slots, P, prev, nxt, expanded, external))
        lst, pairs, runs = _model(mode, slots, prev, nxt, expanded, external)
        assert len(lst) <= 4 * P and len(lst) % 2 == 0 and all(r[1] % 2 == 0 for r in runs)
        want[name] = {"list": " ".join(map(str, lst)), "map": " ".join("(%d,%d)" % p for p in pairs),
                      "runs": " ".join("{%d,%d,%d}" % r for r in runs)}
    got = _plan(tmp_path, lines)
    wrong = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not wrong, sorted(wrong.items())[:5]
