"""The stream contract of every exported entry point that takes a `void *stream`, on streams that are not the null stream
(the rest of the suite launches on the null stream, which serialises everything and so hides every breach):

  T1  everything a call enqueues rides the caller's stream -- kernels, memsets, table builds, the wrappers' temporaries;
  T2  the call returns at once (the documented exceptions carry the line that says so: stream_cases.Case.blocking_doc);
  T3  launch sequences of one context issued on two streams are ordered behind each other (ws_open / ws_wait / ws_close of
      btrapz_host.hip, DESIGN.md "The host driver's structure");
  T4  the context's caches (M'QM table by weights, the sets' tables by content) hold across streams;
  T5  parameter sets that change every step cost no host synchronisation for the first two changes;
  T6  a reader of the context's records on another stream holds back the next writer.

The method: a device-side delay (torch.cuda._sleep) in front of the work on a side stream.  Whatever part of that work runs
on ANOTHER stream runs during the delay -- and then sees the decoy inputs Y (stream_cases.py: valid inputs, so nothing goes
out of bounds) instead of X, or an event it should have waited for not yet signalled.  Outputs are compared bit for bit with the
null-stream run of the same call.  No test lets two launch sequences overlap: where a hand-over is missing, the second sequence
simply runs inside the first one's delay, and the two still never run at the same time."""
import traceback

import numpy as np
import pytest

import stream_cases as SC

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in SC.CASES]
WORKSPACE = [c.name for c in SC.CASES if c.workspace]
DELAY_MIN_MS, DELAY_MAX_MS, DELAY_FACTOR = 20.0, 200.0, 100.0


class World:
    """One solver, two side streams, every case built and run once on the null stream (reference, warm-up and duration),
    and the calibrated delay."""

    def __init__(self):
        import torch
        from spectral_amd.solver import BatchSolver
        self.torch = torch
        self.solver = BatchSolver(0)
        self.dev = self.solver.device
        self.A, self.B = torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev)
        self.inst, self.twins, self.failed, self.ms, self.measured = {}, {}, {}, {}, {}
        for c in SC.CASES:
            try:
                self.inst[c.name] = self.build(c)
                self.ms[c.name] = self.duration(self.inst[c.name])
            except Exception as e:
                if "HIP error" in str(e) or "hipError" in str(e) or "illegal memory access" in str(e):
                    raise                  # (a device fault: nothing more is started on this device)
                self.failed[c.name] = traceback.format_exc()
        self.small()
        self.calibrate()

    def build(self, c):
        """The instance of a case, warmed up on both side streams as well (their allocator pools, the workspaces)."""
        torch = self.torch
        inst = SC.Instance(self.solver, c)
        for s in (self.A, self.B):
            with torch.cuda.stream(s):
                inst.load(inst.X)
                inst.run()
            s.synchronize()
        torch.cuda.synchronize()
        return inst

    def get(self, name):
        if name in self.failed:
            pytest.fail("the case could not be built:\n" + self.failed[name])
        return self.inst[name]

    def twin(self, name):
        """A second instance of the same case (its own inputs, working tensors and outputs): the other sequence of T3."""
        if name not in self.twins:
            self.twins[name] = self.build(SC.by_name(name))
        return self.twins[name]

    def duration(self, inst):
        """Device time of one call on the null stream, ms."""
        torch = self.torch
        inst.load(inst.X)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); inst.run(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def sleep_ms(self, cycles):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.A):
            e0.record(); torch.cuda._sleep(int(cycles)); e1.record()
        self.A.synchronize()
        return e0.elapsed_time(e1)

    def calibrate(self):
        """The cycle count of the delay: at least DELAY_MIN_MS and DELAY_FACTOR x the longest call, at most DELAY_MAX_MS."""
        self.longest = max(self.ms.values()) if self.ms else 0.0
        self.target_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * self.longest))
        # The cycles are the shader clock's, which moves with the load (seen: 0.5 GHz on the first probe, 2.4 GHz later): the
        # count is corrected until a delay of the full length, measured, lands on the target.
        cycles, ms = 1_000_000, 0.0
        for _ in range(12):
            ms = self.sleep_ms(cycles)
            if 0.95 * self.target_ms <= ms <= 1.25 * self.target_ms:
                break
            cycles = int(cycles * min(10.0, self.target_ms / max(ms, 1e-3))) + 1
        self.cycles, self.delay_ms = cycles, self.sleep_ms(cycles)
        print("\n[streams] longest null-stream call %.3f ms (%s); delay target %.1f ms = %d cycles of torch.cuda._sleep, measured %.1f ms"
              % (self.longest, max(self.ms, key=self.ms.get) if self.ms else "-", self.target_ms, self.cycles, self.delay_ms))
        assert self.delay_ms >= 0.9 * self.target_ms, (self.delay_ms, self.target_ms)

    def delay(self):
        """The delay, on the current stream."""
        self.torch.cuda._sleep(self.cycles)

    def small(self):
        """What makes the caches stale: a small batch solved under a weight row and a list of sets no case uses."""
        import torch
        from spectral_amd import synth
        batch, sh = synth.make_batch(8, 10, config=2)
        self.small_db = self.solver.upload(batch)
        self.small_sh = SC.far_shared(sh)
        self.small_sh.w_s = tuple(1.5 * w for w in self.small_sh.w_s)
        self.small_sets = SC.four_sets(sh, shift=0.375)
        self.small_idx = torch.from_numpy(SC.set_index(8, 0)).to(self.dev)
        self.small_out = self.solver.new_result(8, 10)

    def stale(self):
        """T1(b): after this the M'QM table and the sets' tables are rebuilt inside the next call of a case."""
        self.solver.solve(self.small_db, self.small_sh, out=self.small_out)
        self.solver.solve_sets(self.small_db, self.small_sets, self.small_idx, out=self.small_out)
        self.torch.cuda.synchronize()

    def behind_the_delay(self, name):
        """T1(b)-(e), once per case: (the outputs' bits, whether the call returned before the delay had ended)."""
        if name not in self.measured:
            torch, inst = self.torch, self.get(name)
            self.stale()
            inst.load(inst.Y)
            torch.cuda.synchronize()
            with torch.cuda.stream(self.A):
                self.delay()
                gate = torch.cuda.Event(); gate.record()
                inst.load(inst.X)
                outs = inst.run()
                early = not gate.query()
                snap = SC.snapshot(outs)
            self.A.synchronize()
            torch.cuda.synchronize()
            self.measured[name] = (SC.bits(snap), early)
        return self.measured[name]


@pytest.fixture(scope="module")
def world():
    return World()


def differing(got, want):
    return [k for k in want if got.get(k) != want[k]]


def test_premise_a_side_stream_does_not_serialise_with_the_null_stream(world):
    """A flag set behind the delay on a side stream is still unset for the null stream: without that nothing below proves
    anything (a failure, not a skip)."""
    torch = world.torch
    flag = torch.zeros(1, dtype=torch.int32, device=world.dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(world.A):
        world.delay()
        flag.fill_(1)
    seen = flag.clone()                       # (the null stream, at once)
    torch.cuda.synchronize()
    assert int(seen[0]) == 0 and int(flag[0]) == 1, "the side stream and the null stream serialise: the delay hides nothing"
    assert world.delay_ms >= DELAY_MIN_MS * 0.9 and world.delay_ms >= min(DELAY_MAX_MS, DELAY_FACTOR * world.longest) * 0.9


@pytest.mark.parametrize("name", NAMES)
def test_t1_everything_rides_the_callers_stream(world, name):
    """Inputs hold the decoy until, behind the delay and in stream order, X is copied in: the outputs are the null-stream
    run's bit for bit (sentinel regions included) only if every piece of the call waited for that copy."""
    inst = world.get(name)
    got, _ = world.behind_the_delay(name)
    assert not differing(got, inst.R), (name, differing(got, inst.R), "== the decoy's: %s" % [k for k in got if got[k] == inst.RY.get(k)])


@pytest.mark.parametrize("name", NAMES)
def test_t2_the_call_returns_at_once(world, name):
    """The event recorded right behind the delay has not happened when the call returns."""
    case = SC.by_name(name)
    world.get(name)
    _, early = world.behind_the_delay(name)
    if case.asynchronous:
        assert early, (name, "the call came back only after the delay (%.0f ms) had ended: it waits for the device" % world.delay_ms)
    else:
        assert case.blocking_doc.strip(), name


@pytest.mark.parametrize("name", WORKSPACE)
def test_t3_sequences_of_one_context_on_two_streams_are_ordered(world, name):
    """Sequence 1 behind the delay on stream A, sequence 2 right after it on stream B: when 2 has finished, 1 has."""
    torch = world.torch
    one, two = world.get(name), world.twin(name)
    world.stale()
    one.load(one.X); two.load(two.Y)
    torch.cuda.synchronize()
    with torch.cuda.stream(world.A):
        world.delay()
        snap1 = SC.snapshot(one.run())
        eA = torch.cuda.Event(); eA.record()
    with torch.cuda.stream(world.B):
        snap2 = SC.snapshot(two.run())
        eB = torch.cuda.Event(); eB.record()
    eB.synchronize()
    ordered = eA.query()
    torch.cuda.synchronize()
    assert ordered, (name, "the sequence on stream B finished before the one issued before it on stream A: no hand-over of the workspace")
    assert not differing(SC.bits(snap1), one.R) and not differing(SC.bits(snap2), two.RY), (name, differing(SC.bits(snap1), one.R),
                                                                                              differing(SC.bits(snap2), two.RY))


def uniform_pair(world):
    """Two uniform batches on the device, their Shared, result records."""
    torch, solver = world.torch, world.solver
    (a1, sh), (a2, _) = SC.both(lambda seed: SC.scenario(SC.GB, SC.GS, seed))
    dev = lambda a: SC.rec_of({k: torch.from_numpy(v).to(world.dev) for k, v in a.items()}, SC.GB, SC.GS)
    return dev(a1), dev(a2), sh, solver.new_result(SC.GB, SC.GS), solver.new_result(SC.GB, SC.GS)


def solved_bits(world, o):
    world.torch.cuda.synchronize()
    return SC.bits({k: o[k] for k in ("ctrl", "cost", "status", "iters")})


def test_t4_the_weights_table_holds_across_streams(world):
    """A: delay, solve under W1 (the table is rebuilt on A).  B: a solve under W1 -- a cache hit, nothing rebuilt -- must
    read W1's table, not W0's."""
    torch, solver = world.torch, world.solver
    d1, d2, w0, o1, o2 = uniform_pair(world)
    w1 = SC.far_shared(w0)
    want = solved_bits(world, solver.solve(d2, w1, out=o2))
    under_w0 = solved_bits(world, solver.solve(d2, w0, out=o2))
    assert want != under_w0
    solver.solve(d1, w0, out=o1)                      # warm-up under W0
    torch.cuda.synchronize()
    with torch.cuda.stream(world.A):
        world.delay()
        solver.solve(d1, w1, out=o1)
    with torch.cuda.stream(world.B):
        solver.solve(d2, w1, out=o2)
    got = solved_bits(world, o2)
    assert got != under_w0, "the solve on B read the table of the weights before"
    assert got == want


@pytest.mark.parametrize("reader", ["solve_sets", "traj_cost"])
def test_t4_the_sets_tables_hold_across_streams(world, reader):
    """The same with parameter sets (S0 -> S1) through btrapz_solve_sets_device, and with btrapz_traj_cost_device reading
    the sets' cache."""
    torch, solver = world.torch, world.solver
    d1, d2, sh, o1, o2 = uniform_pair(world)
    # (S1: other limits and reference speeds, and the sets in another order -- every candidate gets other weights too)
    s0, s1 = SC.four_sets(sh), SC.four_sets(sh, shift=0.25)[::-1]
    idx = torch.from_numpy(SC.set_index(SC.GB, 1)).to(world.dev)
    s_ref, l_ref = (torch.from_numpy(a).to(world.dev) for a in SC.reference_lines(SC.GB, SC.GS, 1))
    if reader == "solve_sets":
        call = lambda sets: solver.solve_sets(d2, sets, idx, out=o2)
        grab = lambda r: solved_bits(world, r)
    else:
        solver.solve_sets(d2, s0, idx, out=o2)
        torch.cuda.synchronize()
        ctrl, status = o2["ctrl"].clone(), o2["status"].clone()
        call = lambda sets: solver.traj_cost(d2, sets, ctrl, s_ref, l_ref, status=status, set_index=idx)
        grab = lambda r: (torch.cuda.synchronize(), SC.bits(dict(a_cost=r[0], n_points=r[1])))[1]
    want = grab(call(s1))
    under_s0 = grab(call(s0))
    assert want != under_s0
    solver.solve_sets(d1, s0, idx, out=o1)            # warm-up under S0
    torch.cuda.synchronize()
    with torch.cuda.stream(world.A):
        world.delay()
        solver.solve_sets(d1, s1, idx, out=o1)
    with torch.cuda.stream(world.B):
        r = call(s1)
    got = grab(r)
    assert got != under_s0, "the call on B read the tables of the sets before"
    assert got == want


def test_t5_sets_that_change_every_step_cost_no_host_synchronisation(world):
    """Six btrapz_solve_sets_device steps behind one delay, each under another list of sets, into six records: every record is
    its null-stream solve's, and the first two steps -- the two staging buffers of sets_tables -- return before the delay ends."""
    torch, solver = world.torch, world.solver
    d1, _, sh, _, _ = uniform_pair(world)
    idx = torch.from_numpy(SC.set_index(SC.GB, 0)).to(world.dev)
    lists = [SC.four_sets(sh, shift=0.0625 * (i + 1)) for i in range(6)]
    outs = [solver.new_result(SC.GB, SC.GS) for _ in lists]
    want = [solved_bits(world, solver.solve_sets(d1, sets, idx, out=o)) for sets, o in zip(lists, outs)]
    assert len(set(w["ctrl"] for w in want)) == 6
    world.stale()
    for o in outs:
        for v in o.values():
            v.zero_()
    torch.cuda.synchronize()
    early = []
    with torch.cuda.stream(world.A):
        world.delay()
        gate = torch.cuda.Event(); gate.record()
        for sets, o in zip(lists, outs):
            solver.solve_sets(d1, sets, idx, out=o)
            early.append(not gate.query())
    got = [solved_bits(world, o) for o in outs]
    assert got == want, [i for i in range(6) if got[i] != want[i]]
    assert early[0] and early[1], early


def test_t6_a_reader_on_another_stream_holds_back_the_next_writer(world):
    """btrapz_rescue_violations_device behind a delay on stream B; the next rescue solve, on stream A, clears and rewrites the
    records it reads: it must wait for the read."""
    torch, solver = world.torch, world.solver
    n = SC.UB
    (a1, sh), (a2, _) = SC.both(lambda seed: SC.scenario(n, SC.US, seed, damaged=8))
    d1, d2 = (SC.rec_of({k: torch.from_numpy(v).to(world.dev) for k, v in a.items()}, n, SC.US) for a in (a1, a2))
    o1, o2 = solver.new_result(n, SC.US), solver.new_result(n, SC.US)
    v1 = torch.zeros(n, 4, dtype=torch.float64, device=world.dev); out = torch.zeros_like(v1)
    options = dict(elastic=1, lean=-1, split=-1, cap_iter=-1)
    torch.cuda.synchronize()
    with torch.cuda.stream(world.A):
        solver.solve(d1, sh, out=o1, **options)
        solver.ctx.rescue_violations_device(n, v1, stream=solver._stream())
    world.A.synchronize()
    want = SC.bits(dict(viol=v1))
    assert np.nanmax(np.frombuffer(want["viol"])) > 0.0      # (the damaged candidates were rescued: there is something to read)
    with torch.cuda.stream(world.B):
        world.delay()
        solver.ctx.rescue_violations_device(n, out, stream=solver._stream())
        eB = torch.cuda.Event(); eB.record()
    with torch.cuda.stream(world.A):
        solver.solve(d2, sh, out=o2, **options)
        eA = torch.cuda.Event(); eA.record()
    eA.synchronize()
    ordered = eB.query()
    torch.cuda.synchronize()
    assert ordered, "the solve on A finished while the reader on B was still waiting to read the records it rewrites"
    assert SC.bits(dict(viol=out)) == want
