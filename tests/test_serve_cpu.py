"""CPU checks of serving.SlotScheduler, the pure part of Zonos.serve(): FIFO admission by ticket into the lowest free
slot, capacity errors, cancellation, ticket bookkeeping, thread safety and wait_for_work. The scheduler takes no engine;
FakeEngine here plays run_round()'s engine side: a request runs ceil(max_new_tokens / CHUNK) rounds in its slot."""
import threading
import time

import pytest

from zonos_vibes_amd.serving import SlotScheduler, size_buckets

CHUNK = 4
COND = (2, 10, 512)


class FakeEngine:
    """ServeSession.run_round() without a GPU: begin_round, `CHUNK` frames for every busy slot, finish the ended."""

    def __init__(self, sched: SlotScheduler):
        self.sched = sched
        self.left = {}       # slot -> frames left
        self.log = []        # (round, "admit" | "release", slot, ticket or None)
        self.round_no = 0

    def run_round(self):
        if self.sched.idle:
            return []
        self.round_no += 1
        released, admitted = self.sched.begin_round()
        for s in released:
            self.log.append((self.round_no, "release", s, None))
            del self.left[s]
        for s, r in admitted:
            self.log.append((self.round_no, "admit", s, r.ticket))
            self.left[s] = r.max_new_tokens
        items = []
        for s, r in self.sched.busy():
            n = min(CHUNK, self.left[s])
            self.left[s] -= n
            last = self.left[s] == 0
            if last:
                del self.left[s]
                self.sched.finish(s)
            items.append((r.ticket, n, last))
        return items

    def admitted(self):
        return [(rnd, s, t) for rnd, what, s, t in self.log if what == "admit"]


def _sched(slots=2):
    return SlotScheduler(slots, max_seqlen=128, max_prefill=64, d_model=512)


def test_tickets_count_up_and_admission_is_fifo_into_the_lowest_free_slot():
    sc = _sched(2)
    eng = FakeEngine(sc)
    assert sc.idle and eng.run_round() == []
    tickets = [sc.submit(COND, None, m) for m in (12, 4, 8, 8)]  # rounds: 3, 1, 2, 2
    assert tickets == [0, 1, 2, 3] and not sc.idle
    items = []
    while not sc.idle:
        items += eng.run_round()
    # round 1: tickets 0, 1 into slots 0, 1; ticket 1 ends in round 1, so slot 1 goes to ticket 2 in round 2; ticket 0
    # (slot 0) and ticket 2 (slot 1) both end in round 3, and the one waiting ticket takes the LOWEST free slot
    assert eng.admitted() == [(1, 0, 0), (1, 1, 1), (2, 1, 2), (4, 0, 3)]
    for t, m in zip(tickets, (12, 4, 8, 8)):
        mine = [(n, last) for tk, n, last in items if tk == t]
        assert sum(n for n, _ in mine) == m and [last for _, last in mine].count(True) == 1 and mine[-1][1]
    assert eng.run_round() == []


def test_a_request_is_admitted_only_when_a_slot_frees():
    sc = _sched(1)
    eng = FakeEngine(sc)
    sc.submit(COND, None, 12)
    sc.submit(COND, None, 4)
    for _ in range(3):
        assert {t for t, _, _ in eng.run_round()} == {0}
    assert eng.admitted() == [(1, 0, 0)]
    assert eng.run_round() == [(1, 4, True)]
    assert eng.admitted() == [(1, 0, 0), (4, 0, 1)] and sc.idle


@pytest.mark.parametrize("cond, prefix, mnt", [
    ((2, 10, 512), None, 110),           # Lc + P + n + 9 = 129 > max_seqlen 128
    ((2, 10, 512), (1, 9, 20), 90),      # with the prefix: 10 + 20 + 90 + 9 = 129
    ((2, 64, 512), None, 5),             # Lc + P + 1 = 65 > max_prefill 64
    ((2, 40, 512), (1, 9, 24), 5),       # 40 + 24 + 1 = 65
    ((1, 10, 512), None, 5),             # not a (cond, uncond) pair
    ((2, 10, 256), None, 5),             # wrong d_model
    ((2, 10), None, 5),
    ((2, 10, 512), (1, 8, 4), 5),        # not 9 codebooks
    ((2, 10, 512), None, 0),
])
def test_submit_capacity_errors_leave_the_queue_untouched(cond, prefix, mnt):
    sc = _sched(1)
    assert sc.submit(COND, None, 109) == 0 and sc.submit(COND, (1, 9, 20), 89) == 1  # exactly at the limits: fit
    assert sc.submit((2, 63, 512), None, 5) == 2
    with pytest.raises(ValueError):
        sc.submit(cond, prefix, mnt)
    assert sc.submit(COND, None, 4) == 3  # no ticket was used up
    _, admitted = sc.begin_round()
    assert [(s, r.ticket) for s, r in admitted] == [(0, 0)]
    assert [r.ticket for r in sc._waiting] == [1, 2, 3]


def test_cancel_of_a_waiting_ticket_never_starts():
    sc = _sched(1)
    eng = FakeEngine(sc)
    for m in (8, 8, 4):
        sc.submit(COND, None, m)
    eng.run_round()
    assert sc.cancel(1) is True and sc.cancel(1) is False
    items = []
    while not sc.idle:
        items += eng.run_round()
    assert {t for t, _, _ in items} == {0, 2}
    assert [t for _, _, t in eng.admitted()] == [0, 2]


def test_cancel_of_a_running_ticket_frees_its_slot_for_the_next_waiting_one():
    sc = _sched(2)
    eng = FakeEngine(sc)
    for m in (40, 40, 8, 8):
        sc.submit(COND, None, m)
    first = eng.run_round()
    assert {t for t, _, _ in first} == {0, 1}
    assert sc.cancel(0) is True and sc.cancel(0) is False  # already cancelled
    assert sc.is_cancelled(0)
    items = eng.run_round()
    assert (2, "release", 0, None) in eng.log
    assert eng.admitted()[-1] == (2, 0, 2)  # slot 0 went to ticket 2, the next one waiting
    assert {t for t, _, _ in items} == {1, 2} and not sc.is_cancelled(0)
    while not sc.idle:
        items += eng.run_round()
    assert 0 not in {t for t, _, _ in items}
    assert sorted(t for t, _, last in items if last) == [1, 2, 3]


def test_cancel_of_a_finished_or_unknown_ticket_is_false():
    sc = _sched(1)
    eng = FakeEngine(sc)
    assert sc.cancel(0) is False and sc.cancel(-1) is False  # nothing submitted yet
    t = sc.submit(COND, None, 4)
    assert eng.run_round() == [(t, 4, True)]
    assert sc.cancel(t) is False and sc.cancel(7) is False and sc.idle


def test_close_drops_everything_and_refuses_submits():
    sc = _sched(2)
    eng = FakeEngine(sc)
    for m in (40, 40, 8):
        sc.submit(COND, None, m)
    eng.run_round()
    assert sc.release_all() == [0, 1] and sc.idle
    with pytest.raises(RuntimeError):
        sc.submit(COND, None, 4)


def test_four_threads_submit_while_the_main_thread_drains():
    sc = _sched(3)
    eng = FakeEngine(sc)
    got, errors = [[] for _ in range(4)], []

    def client(k):
        try:
            for j in range(50):
                got[k].append(sc.submit(COND, None, 1 + (7 * k + j) % 9))
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=client, args=(k,)) for k in range(4)]
    for th in threads:
        th.start()
    items = []
    while any(th.is_alive() for th in threads) or not sc.idle:
        items += eng.run_round()
    for th in threads:
        th.join()
    while not sc.idle:
        items += eng.run_round()
    assert not errors
    tickets = sorted(t for g in got for t in g)
    assert tickets == list(range(200))                       # every submit got a ticket of its own, counting up
    assert all(g == sorted(g) for g in got)                  # and each thread saw them ascend
    assert sorted(t for _, _, t in eng.admitted()) == tickets  # served exactly once
    assert sorted(t for t, _, last in items if last) == tickets  # exactly one `last` each
    order = [t for _, _, t in eng.admitted()]
    assert order == sorted(order)                            # FIFO by ticket


def test_wait_for_work_returns_on_a_submit_and_times_out_otherwise():
    sc = _sched(1)
    t0 = time.monotonic()
    assert sc.wait_for_work(timeout=0.05) is False
    assert time.monotonic() - t0 >= 0.04
    th = threading.Timer(0.05, lambda: sc.submit(COND, None, 4))
    th.start()
    assert sc.wait_for_work(timeout=10.0) is True
    th.join()
    assert time.monotonic() - t0 < 5.0
    assert sc.wait_for_work(timeout=0) is True  # work is waiting: at once


def test_size_buckets_are_stream_batch_s():
    assert size_buckets(3) == [1, 2, 3] and size_buckets(64) == [1, 2, 4, 8, 16, 24, 32, 40, 48, 56, 64]
