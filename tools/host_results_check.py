"""The scenarios of the executor's host results in which a call could block: run as a child process with a time limit by
tests/test_gpu_host_results.py, so that a deadlock fails instead of hanging the suite.  One `ok <scenario>` line each.

  error-batch       a batch that fails before its scan (a rescan in a context that holds no pages yet, as tools/gate_check.py provokes
                    it) between two good ones, fetch on: host_results raises that batch's error, its neighbours deliver
  release-order-1   focr_fleet_submit refuses ("release the oldest") while the context the new ticket maps to holds an unreleased
                    batch, however many OTHER tickets were released: one device, four contexts, tickets 1-4 out, 2 released.
                    Before the fix of fleet.hip (a count of releases) this submit waited for ticket 1's release on the thread that
                    would have had to make it: run it against a fixed library only
  release-order-2   the same on a fleet of two executors, with the refused ticket and the one in its way on the second executor
  two-consumers     two threads ask for the same ticket's host results at once, and for two different tickets at once: one of them
                    completes the batch, both get the same record
Expected results come from the oracle (tests/executor_cases.py), never from the library."""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import executor_cases as EC  # noqa: E402
from font_ocr_amd.searcher import SCAN_MFMA, Fleet, FocrError, Pipeline  # noqa: E402

bank, cases, exp = EC.all_expected()


def same(rec, e, what):
    assert (rec.n_pages, rec.n_templates, rec.n_matches, rec.n_lines, rec.n_chars) == (e.n_pages, e.n_templates, e.n_matches, e.n_lines, e.n_chars), what
    assert rec.counts.tobytes() == e.counts.tobytes(), f"{what}: counts"
    assert rec.page_line_off.tobytes() == e.page_line_off.tobytes(), f"{what}: page_line_off"
    assert rec.line_char_off.tobytes() == e.line_char_off.tobytes(), f"{what}: line_char_off"
    assert rec.lines_flat_bytes() == e.chars.tobytes(), f"{what}: chars"


def args(name):
    c = cases[name]
    return (c["pages"], c["thr"], c["cap"], SCAN_MFMA, True, c["anchor"], c["overlap"])


def error_batch():
    pipe = Pipeline(0, 3)
    try:
        pipe.set_bank(bank)
        pipe.set_fetch(True)
        t1 = pipe.submit(*args("text"))
        c = cases["text"]
        t2 = pipe.submit(None, c["thr"], c["cap"])  # context 2 holds no pages yet: fails before any kernel
        t3 = pipe.submit(*args("one-blank-page"))
        try:
            pipe.host_results(t2)
            raise AssertionError("the rescan of an empty context delivered")
        except FocrError as e:
            assert "no pages resident" in str(e), str(e)
        try:
            pipe.host_results(t2)  # asked again (the DONE path): the same error, not a stale record
            raise AssertionError("the failed batch delivered at the second call")
        except FocrError as e:
            assert "no pages resident" in str(e), str(e)
        pipe.release(t2)
        same(pipe.host_results(t3), exp["one-blank-page"], "the ticket behind the failed one")
        same(pipe.host_results(t1), exp["text"], "the ticket in front of the failed one")
        pipe.release(t3)
        pipe.release(t1)
        t4 = pipe.submit(*args("cap1"))
        same(pipe.host_results(t4), exp["cap1"], "the next ticket")
        pipe.release(t4)
    finally:
        pipe.close()


def release_order(devices, first_release, stray, blocker):
    """Fill every context; release `first_release` in order (each followed by a submit that must succeed), then `stray` out of order:
    the next submit maps to `blocker`'s context and must be refused until `blocker` is released."""
    kinds = ("text", "one-blank-page", "cap1", "odd-width", "dword-width", "no-lines", "blank", "text", "cap1", "one-blank-page", "text", "cap1")
    fl = Fleet(devices, lanes=2)
    try:
        fl.set_bank(bank)
        fl.set_fetch(True)
        name_of = {}

        def submit():
            k = kinds[len(name_of)]
            t = fl.submit(*args(k))
            name_of[t] = k
            return t

        released = set()

        def retire(t, what):
            same(fl.host_results(t), exp[name_of[t]], what)
            fl.release(t)
            released.add(t)

        for k in range(fl.slots):
            assert submit() == k + 1
        for t in first_release:
            retire(t, f"ticket {t}")
            assert submit() == len(name_of)
        retire(stray, f"ticket {stray}, out of order")
        nxt = len(name_of) + 1
        assert nxt - fl.slots == blocker and blocker not in released and fl.device_of(nxt) == fl.device_of(blocker)
        for _ in range(2):  # (a refused submit takes no ticket)
            try:
                submit()
                raise AssertionError(f"ticket {nxt} was handed out while ticket {blocker} holds its context")
            except FocrError as e:
                assert "release the oldest" in str(e), str(e)
        retire(blocker, f"ticket {blocker}")
        while len(name_of) < stray + fl.slots:  # on to the ticket that takes the context the stray one left
            t = len(name_of) + 1
            if t - fl.slots not in released:
                retire(t - fl.slots, f"ticket {t - fl.slots}")
            assert submit() == t
            same(fl.host_results(t), exp[name_of[t]], f"ticket {t} after the release")
        for t in sorted(set(name_of) - released):
            retire(t, f"ticket {t} at the end")
    finally:
        fl.close()


def two_consumers():
    pipe = Pipeline(0, 3)
    try:
        pipe.set_bank(bank)
        pipe.set_fetch(True)
        ta, tb = pipe.submit(*args("big")), pipe.submit(*args("dense"))
        got, errs = {}, []

        def ask(key, t):
            try:
                got[key] = pipe.host_results(t)
            except Exception as e:  # noqa: BLE001
                errs.append(repr(e))

        th = [threading.Thread(target=ask, args=(k, t), daemon=True) for k, t in (("a1", ta), ("a2", ta), ("b1", tb), ("b2", tb))]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=60)
            assert not t.is_alive(), "a consumer thread is stuck"
        assert not errs, errs
        for k, name in (("a1", "big"), ("a2", "big"), ("b1", "dense"), ("b2", "dense")):
            same(got[k], exp[name], k)
        assert got["a1"].addresses == got["a2"].addresses and got["b1"].addresses == got["b2"].addresses
        pipe.release(ta)
        pipe.release(tb)
    finally:
        pipe.close()


if __name__ == "__main__":
    error_batch()
    print("ok error-batch", flush=True)
    # one device, 4 contexts: 1-4 out, 2 released out of order; ticket 5 maps to ticket 1's context
    release_order([0], first_release=(), stray=2, blocker=1)
    print("ok release-order-1", flush=True)
    # two executors, 8 contexts: 1 released in order and 9 submitted; 4 released out of order; ticket 10 maps to ticket 2's context,
    # on the second executor
    release_order([0, 0], first_release=(1,), stray=4, blocker=2)
    print("ok release-order-2", flush=True)
    two_consumers()
    print("ok two-consumers", flush=True)
