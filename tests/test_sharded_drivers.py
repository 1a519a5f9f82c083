"""The two generic drivers of noize_job_amd.sharded behind run_hydraulic / run_fluvial / run_fill and their lockstep forms,
on toy generators: no kernels, no process group.  A request is (planes, up_rows, down_rows) for an exchange or (VOTE, word)
for a vote; the drivers answer an exchange with None and a vote with the maximum of every rank's word."""
import pytest
import torch

from noize_job_amd import sharded as sh


def word(v):
    return torch.tensor([v], dtype=torch.int32)


def script(steps, log, value):
    """A generator that yields `steps` in turn, writes down what it was sent back for each, and returns `value`."""
    for req in steps:
        log.append((yield req))
    return value


class Comm:
    """Records the exchanges; a vote is the maximum with the words the other ranks are said to hold."""

    def __init__(self, others=()):
        self.others, self.exchanges = others, []

    def exchange(self, planes, plan, up_rows, down_rows):
        self.exchanges.append((planes, plan, up_rows, down_rows))

    def allreduce_max(self, words):
        words.fill_(max([int(words[0])] + list(self.others)))
        return int(words[0])


def test_run_steps_serves_exchanges_and_votes_and_returns_the_value():
    comm, log, w = Comm(others=(5, 2)), [], word(3)
    got = sh._run_steps(script([(["A"], 1, 2), (sh.VOTE, w), (["B", "C"], 0, 4)], log, ("plane", 7)), comm, "plan")
    assert got == ("plane", 7)
    assert comm.exchanges == [(["A"], "plan", 1, 2), (["B", "C"], "plan", 0, 4)]
    assert log == [None, 5, None] and int(w[0]) == 5
    # a generator that asks for nothing
    assert sh._run_steps(script([], [], "done"), comm, "plan") == "done"


def test_public_drivers_go_through_run_steps(monkeypatch):
    """run_hydraulic / run_fluvial / run_fill hand their stage's generator, the comm and the plan to _run_steps."""
    seen = []
    monkeypatch.setattr(sh, "_run_steps", lambda gen, comm, plan: seen.append((gen.gi_code.co_name, comm, plan)) or "value")
    bufs = dict(A=None, B=None, S0=None, S1=None, D0=None, D1=None, H=None, W=None, work=None, words=None)
    assert sh.run_hydraulic("ops", "comm", "plan", None, bufs, 2) == "value"
    assert sh.run_fluvial("ops", "comm", "plan", None, bufs) == "value"
    assert sh.run_fill("ops", "comm", "plan", None, bufs) == "value"
    assert seen == [(name, "comm", "plan") for name in ("hydraulic_steps", "fluvial_steps", "fill_steps")]


def test_lockstep_vote_reaches_every_word_and_comes_back():
    plans = [sh.StripePlan(r, 3, 30, 4, 1) for r in range(3)]
    logs, words = [[], [], []], [word(0), word(4), word(1)]
    gens = [script([(sh.VOTE, words[r]), (sh.VOTE, words[r])], logs[r], "rank %d" % r) for r in range(3)]
    copies = []
    got = sh._run_steps_lockstep(gens, plans, lambda *a: copies.append(a))
    assert got == ["rank 0", "rank 1", "rank 2"]          # every rank's value, in rank order
    assert [int(w[0]) for w in words] == [4, 4, 4] and logs == [[4, 4]] * 3
    assert copies == []


def test_lockstep_exchange_copies_ghost_rows_and_answers_none():
    plans = [sh.StripePlan(r, 2, 20, 4, 2) for r in range(2)]
    logs = [[], []]
    gens = [script([(["P%d" % r], 2, 1)], logs[r], r) for r in range(2)]
    copies = []
    assert sh._run_steps_lockstep(gens, plans, lambda *a: copies.append(a)) == [0, 1]
    assert logs == [[None], [None]]
    # rank 0's bottom ghost row from rank 1's first owned row; rank 1's two top ghost rows from rank 0's last owned rows
    assert copies == [("P0", plans[0].own1, "P1", plans[1].own0, 1), ("P1", plans[1].own0 - 2, "P0", plans[0].own1 - 2, 2)]


@pytest.mark.parametrize("steps", [
    ([(["A"], 1, 1), (["A"], 1, 1)], [(["B"], 1, 1)]),              # rank 1 ends one request early
    ([], [(["B"], 1, 1)]),                                           # rank 0 asks for nothing at all
    ([(sh.VOTE, word(1))], [(["B"], 1, 1)]),                        # rank 0 votes where rank 1 exchanges
    ([(["A"], 1, 1)], [(sh.VOTE, word(1))]),                        # ... and the other way round
])
def test_lockstep_refuses_ranks_that_leave_the_schedule(steps):
    plans = [sh.StripePlan(r, 2, 20, 4, 1) for r in range(2)]
    gens = [script(s, [], None) for s in steps]
    with pytest.raises(AssertionError, match="ranks left the schedule at different points"):
        sh._run_steps_lockstep(gens, plans, lambda *a: None)


def test_stage_params_defaults_overrides_and_assertion_texts():
    assert sh.hydraulic_params() == sh.HYDRAULIC_DEFAULTS and sh.fluvial_params() == sh.FLUVIAL_DEFAULTS
    assert sh.hydraulic_params(dict(rain=2.0), iterations=3) == dict(sh.HYDRAULIC_DEFAULTS, rain=2.0, iterations=3)
    assert sh.fluvial_params(dict(dt=0.5), dt=0.25)["dt"] == 0.25            # keyword arguments win
    assert sh.HYDRAULIC_DEFAULTS["rain"] == 1e-4 and sh.FLUVIAL_DEFAULTS["dt"] == 1.0   # the defaults are not written to
    with pytest.raises(AssertionError, match="^wear is not a scalar field of nz_hydraulic_desc$"):
        sh.hydraulic_params(wear=1)
    with pytest.raises(AssertionError, match="^rainMap is not a scalar field of nz_fluvial_desc$"):
        sh.fluvial_params(dict(rainMap=1))
    with pytest.raises(AssertionError, match="^depth is not a parameter of the sharded fill$"):
        next(sh.fill_steps(None, None, dict(depth=1), dict(words=None)))
