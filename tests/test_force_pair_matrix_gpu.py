"""GPU: every single-system force loop, one (row, column) pair term at a time (tests/force_pair_ref.py states the inputs,
the reference, the tolerance and the table of cases; tests/test_force_pair_matrix_cpu.py ties each case to its kernels).

One NBodySystem per case, the base state kept on the device.  Per source: positions and mass words restored, velocities
zeroed, step(1.0, eps, sync=False), the new velocities -- the force pass' sums themselves -- copied into a device-side
buffer, downloaded in chunks.  Parts of a case:
  (A) one source, equal-mass path on, then off: every row against its single fp64 term within K u of it; the source's own
      row, the row lying on the source and every row of the all-zero-mass run are 0 bit for bit, up to the sign of zero;
  (B) the source's split lit with its companions far away, path on, then off: the same terms through the equal-mass loops;
      where the case has such a loop the two runs must differ in some bit (the switch took the other loop), where it has
      none (eps = 0: the guarded loops, and the compiler-scheduled general kernel) it is only reported;
  (C) where the table says so, a lit near set (a whole split, or a 128-body window of one): every row's sum within its
      row-level tolerance -- the equal-mass diagonal squares, where a single term cannot be isolated;
  (E) the other one-sided blockings: bit-equal to blocking 4, entry for entry.
Mass words and fourth velocity words come back untouched; everything is finite, the far rows included.  The worst
|gpu - ref| / tol and the seconds of every case are printed; profiles/force_pair_matrix.txt records them."""
import time

import numpy as np
import pytest

import force_pair_ref as fp

pytestmark = pytest.mark.gpu

CHUNK_ENTRIES = 1 << 21        # (source, row) entries checked, and downloaded, at a time


@pytest.fixture(scope="module")
def nb():
    import torch
    import n_body_problem_amd as nb
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    return nb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Runner:
    """The system of one case and its device-side states."""

    def __init__(self, nb, case):
        import torch
        self.torch, self.case = torch, case
        n = self.n = case["n"]
        self.x = fp.configuration(n)
        self.eps_pp = fp.softening_lengths(n) if case["pps"] else None
        self.K = fp.k_of(case["pps"])
        self.s = nb.NBodySystem(n, split_len=case["split_len"])
        self.s.set_force_mode(case["mode"])
        if case["rows_per_lane"]:
            self.s.set_rows_per_lane(case["rows_per_lane"])
        if case["strip"]:
            self.s.set_strip_len(case["strip"])
        if case["pps"]:
            self.s.set_particle_softening(self.eps_pp)
        assert self.s.split_len == case["split_len"]
        dev = self.s.device
        near = np.zeros((n, 4), np.float32)
        near[:, :3] = self.x
        self.dark = torch.from_numpy(near).to(dev)                    # every body in place, every mass word 0
        near[:, 3] = fp.MASS
        self.lit = torch.from_numpy(near).to(dev)                     # every body in place, every mass word MASS
        v0 = np.zeros((n, 4), np.float32)
        v0[:, 3] = fp.W_WORD
        self.v0 = torch.from_numpy(v0).to(dev)
        self.seconds = 0.0

    def close(self):
        self.s.close()

    def step(self):
        self.s.velocities.copy_(self.v0)
        self.s.step(1.0, self.case["eps"], sync=False)

    def sweep(self, bases, which, sources, path_on):
        """One step per source c = sources[k] from the base state bases[which[k]] with body c in place and lit.  Returns the
        device tensors (S, n, 4) of new velocities and (S, n) of mass words."""
        torch, s = self.torch, self.s
        s.set_equal_mass_path(path_on)
        out = torch.empty((len(sources), self.n, 4), dtype=torch.float32, device=s.device)
        mass = torch.empty((len(sources), self.n), dtype=torch.float32, device=s.device)
        t0 = time.perf_counter()
        for k, c in enumerate(sources):
            c = int(c)
            s.positions.copy_(bases[which[k]])
            if c >= 0:
                s.positions[c].copy_(self.lit[c])
            self.step()
            out[k].copy_(s.velocities)
            mass[k].copy_(s.positions[:, 3])
        torch.cuda.synchronize(s.device)
        self.seconds += time.perf_counter() - t0
        return out, mass


def chunks(count, n):
    step = max(1, CHUNK_ENTRIES // n)
    return [(a, min(count, a + step)) for a in range(0, count, step)]


def held(run, case, part, out, sources, refs, far_of=None):
    """Every entry of a sweep against its term: the worst ratio, or an AssertionError that names case, source and row."""
    n, name = case["n"], f"{case['name']} ({part})"
    worst = 0.0
    for (a, b), ref in zip(chunks(len(sources), n), refs):
        got = out[a:b].cpu().numpy()
        assert np.isfinite(got).all(), f"{name}: a velocity that is not finite, sources {sources[a]} .. {sources[b - 1]}"
        assert (got[..., 3] == fp.W_WORD).all(), f"{name}: a fourth velocity word changed"
        if far_of is None:
            tol = fp.tolerance(ref, run.K)
        else:                                                           # (B): lo, cnt of the lit split of every source
            far = np.array([cnt - 1 for _, cnt in far_of[a:b]], np.float64)[:, None, None]
            tol = fp.tolerance(ref, run.K, far)
            for k in range(a, b):
                lo, cnt = far_of[k]
                own = tol[k - a, sources[k]].copy()                     # the source's own row: its far companions' terms alone
                tol[k - a, lo:lo + cnt] = np.inf                        # the far companions' own rows: finite, no more
                tol[k - a, sources[k]] = own
        w, fails = fp.check(got[..., :3], ref, tol, name, sources[a:b])
        assert not fails, fp.describe(fails)
        worst = max(worst, w)
    return worst


def mass_words_held(case, part, mass, expected):
    got = mass.cpu().numpy()
    assert np.array_equal(bits(got), bits(expected)), f"{case['name']} ({part}): a mass word changed"


def run_case(nb, case):
    n, L = case["n"], case["split_len"]
    t_case = time.perf_counter()
    run = Runner(nb, case)
    try:
        sources = fp.sources_of(case)
        S = len(sources)
        report = {}
        if "E" in case["parts"]:
            got = {}
            for rpl in (4, case["rows_per_lane"]):
                run.s.set_rows_per_lane(rpl)
                out, _ = run.sweep([run.dark], [0] * S, sources, True)
                got[rpl] = out.cpu().numpy()
            refs = [fp.terms(run.x, sources, case["eps"], run.eps_pp)]
            report["E"] = held(run, case, "E", out, sources, refs)
            differ = np.argwhere(bits(got[4]) != bits(got[case["rows_per_lane"]]))
            assert not len(differ), f"{case['name']}: blocking {case['rows_per_lane']} differs from blocking 4 at source " \
                f"{sources[differ[0][0]]} row {differ[0][1]} word {differ[0][2]}"
        if "A" in case["parts"]:
            refs = [fp.terms(run.x, sources[a:b], case["eps"], run.eps_pp) for a, b in chunks(S, n)]
            # (A) and the all-zero-mass run
            out, _ = run.sweep([run.dark], [0], [-1], True)
            null = out.cpu().numpy()
            assert not null[0, :, :3].any() and (null[0, :, 3] == fp.W_WORD).all(), f"{case['name']}: the all-zero-mass run moves a body"
            single = np.zeros((S, n), np.float32)
            single[np.arange(S), sources] = fp.MASS
            kept = {}
            for path_on in (True, False):
                part = f"A, equal-mass path {'on' if path_on else 'off'}"
                out, mass = run.sweep([run.dark], [0] * S, sources, path_on)
                report[part] = held(run, case, part, out, sources, refs)
                mass_words_held(case, part, mass, single)
                own = out[torch_index(run, np.arange(S)), torch_index(run, sources)].cpu().numpy()
                assert not own[:, :3].any(), f"{case['name']} ({part}): a source moves itself"
                for k, row in ((int(np.flatnonzero(sources == fp.COINCIDENT)[0]), fp.coincident_row(n)),
                               (int(np.flatnonzero(sources == fp.coincident_row(n))[0]), fp.COINCIDENT)):
                    assert not out[k, row, :3].cpu().numpy().any(), f"{case['name']} ({part}): source {sources[k]} moves row {row}, which lies on it"
                del out, mass
            # (B): every split lit in turn, for the sources that belong to it
            spl = fp.splits(n, L)
            bases = [run.torch.from_numpy(fp.lit_state(case, run.x, lo, cnt)).to(run.s.device) for lo, cnt in spl]
            which = [int(c) // L for c in sources]
            far_of = [spl[w] for w in which]
            words = {w: fp.lit_state(case, run.x, *spl[w])[:, 3] for w in sorted(set(which))}
            lit_mass = np.stack([words[w] for w in which])
            for path_on in (True, False):
                part = f"B, equal-mass path {'on' if path_on else 'off'}"
                out, mass = run.sweep(bases, which, sources, path_on)
                report[part] = held(run, case, part, out, sources, refs, far_of)
                mass_words_held(case, part, mass, lit_mass)
                kept[path_on] = out
                del out, mass
            same = bool(run.torch.equal(kept[True].view(run.torch.int32), kept[False].view(run.torch.int32)))
            report["B on and off bit-identical"] = same
            if case["equal_mass_loop"]:
                assert not same, f"{case['name']} (B): the equal-mass switch changed no bit: the lit split did not take the equal-mass loop"
            del kept, bases
        if case["diag"]:
            report["C"] = diagonal_part(run, case)
        seconds = time.perf_counter() - t_case
        print(f"force pair matrix {case['name']}: n {n} split {L} sources {S}: worst |gpu - ref| / tol " +
              ", ".join(f"{k}: {v:.3f}" if isinstance(v, float) else f"{k}: {v}" for k, v in report.items()) +
              f"; {run.seconds:.2f} s on the GPU, {seconds:.2f} s in all")
        assert all(v <= 1.0 for v in report.values() if isinstance(v, float))
    finally:
        run.close()


def torch_index(run, a):
    return run.torch.from_numpy(np.asarray(a, np.int64)).to(run.s.device)


def diagonal_part(run, case):
    """(C): every lit near set of the case in turn, equal-mass path on; the rows' sums against their row-level tolerance."""
    torch, s, n = run.torch, run.s, case["n"]
    sets = fp.lit_sets(case)
    if case["diag"] == "windows":
        L = case["split_len"]
        elsewhere = np.concatenate([np.arange(w * L, w * L + 256) for w in fp.WINDOW_ROWS_ELSEWHERE])
        rows = [np.concatenate([near, elsewhere]) for _, _, near in sets]
    else:
        rows = [np.arange(n) for _ in sets]
    s.set_equal_mass_path(True)
    out = torch.empty((len(sets), len(rows[0]), 4), dtype=torch.float32, device=s.device)
    finite = torch.ones((), dtype=torch.bool, device=s.device)
    far_base = {}
    t0 = time.perf_counter()
    for k, (lo, cnt, near) in enumerate(sets):
        if lo not in far_base:
            far_base[lo] = torch.from_numpy(fp.lit_state(case, run.x, lo, cnt)).to(s.device)
        idx = torch_index(run, near)
        s.positions.copy_(far_base[lo])
        s.positions[idx] = run.lit[idx]
        run.step()
        finite &= torch.isfinite(s.velocities).all()
        out[k].copy_(s.velocities[torch_index(run, rows[k])])
    torch.cuda.synchronize(s.device)
    run.seconds += time.perf_counter() - t0
    assert bool(finite.cpu()), f"{case['name']} (C): a velocity that is not finite"
    got = out.cpu().numpy()
    assert (got[..., 3] == fp.W_WORD).all(), f"{case['name']} (C): a fourth velocity word changed"
    worst = 0.0
    for k, (lo, cnt, near) in enumerate(sets):
        ref, lengths = fp.near_set_sums(run.x, near, rows[k], case["eps"], run.eps_pp)
        tol = fp.row_tolerance(lengths, run.K, len(near), far=cnt - len(near))
        ratio = np.linalg.norm(got[k, :, :3].astype(np.float64) - ref, axis=-1) / tol
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1.0, f"{case['name']} (C): lit bodies {near[0]} .. {near[-1]} ({len(near)}), row {rows[k][i]}: " \
            f"got {got[k, i, :3]!r} ref {ref[i]!r} tol {tol[i]:.3g} (x{ratio[i]:.3g})"
        worst = max(worst, float(ratio[i]))
    return worst


@pytest.mark.parametrize("case", fp.CASES, ids=[c["name"] for c in fp.CASES])
def test_every_pair_term(nb, case):
    run_case(nb, case)
