"""GPU tests of the batched weight-gradient launch (csrc/mlp.hip: weight_grad_batched_kernel +
weight_grad_reduce_batched_kernel) through the C ABI (tests/wgrad_helpers.py: run_jobs): all six kernel variants
(ceil(O/32) x ceil(K/32)) at every width edge, the row counts at which the partition of the rows changes (the 12-row step,
the even rounding of a workgroup's and of a row split's range, one to 256 workgroups, trailing workgroups with few or no
rows), virtual input rows at piece borders anywhere relative to the 32-column tiles, 16 heterogeneous jobs in one launch,
the documented workspace layout, every refused argument, and mlp.weight_grads over more jobs than one launch takes.

Integer inputs (no zeros, every fp32 partial sum an exact integer): the result must equal dz^T @ inp in fp64 bit for bit;
a dropped, doubled or mis-paired row changes every entry, a wrong column, tile, split, partial or job its entry.  Float
inputs: |dw - fp64| <= wgrad_helpers.rounding_bound element by element, the gamma_D bound derived from the partition (not
tuned; tests/test_wgrad_host.py checks it against an fp32 model of the partition).  Every input sits between NaN rows
(guarded), every output and the workspace are NaN before the launch and every output sits between canaries.

Observed on an MI355X, max over the entries of err / bound for the six variants' shapes: N = 1 0.079 .. 0.090, N = 2
0.084 .. 0.146, N = 13 0.061 .. 0.106, N = 257 0.0062 .. 0.0166, N = 513 0.0037 .. 0.0075, N = 4999 0.0010 .. 0.0017;
virtual rows at N = 257, over the six splits and four O: 0.0051 .. 0.0147.  Every integer case is exact.  The float
tests print their figures before they assert.

That the tests bite was shown once with three mutated kernels, each of which only narrows what is read or written:
`ok = row + 1 < w1` in the operand loads fails 64 of the 67 tests (all but the refusals and the two determinism cases,
which compare the kernel with itself), `k < K - 1` in the partial stores fails all 67 (the workspace's NaN prefill
reaches the last column of every dw: the finiteness check of every launch through run_jobs reports it), and `p1 = min(nparts - 1, ..)` in the reduce kernel fails 57: all but those three and the seven cases at
N = 65537, where the last of the 256 workgroups has no rows and its partial is zero."""
import pytest
import torch

from tests import wgrad_helpers as H

pytestmark = pytest.mark.gpu

E_ARG, E_SPACE = 1, 3                                      # include/instag_hip.h
WIDTHS_O = [1, 31, 32, 33, 63, 64]
WIDTHS_K = [1, 31, 32, 33, 63, 64, 65, 95, 96]
VARIANTS = [(32, 32), (31, 33), (1, 96), (33, 31), (64, 64), (63, 65)]      # (O, K), one per kernel variant
# 15 stored-row neighbours of a launch: the six variants and nine more edges
FILLERS = VARIANTS + [(1, 1), (64, 1), (1, 31), (33, 96), (63, 95), (31, 64), (64, 33), (32, 65), (33, 63)]
SPLITS = [(36, 32, 6), (32, 32, 32), (1, 63, 1), (63, 1, 1), (1, 1, 63), (31, 33, 31)]      # (KX, KA, KE)


def _variant(O, K):
    return ((O + 31) // 32, (K + 31) // 32)


def _dev(t):
    return H.guarded(t.cuda())


def _good(run, what):
    assert run.rc == 0, (what, run.rc, run.error)
    assert run.intact, f"{what}: a canary around a dw or behind the workspace was overwritten"
    for i, dw in enumerate(run.dws):
        assert bool(torch.isfinite(dw).all()), f"{what}: job {i} left or read a NaN ({int((~torch.isfinite(dw)).sum())} entries)"


def _assert_exact(dw, ref, what):
    got = dw.cpu().double()
    assert got.shape == ref.shape, what
    if not torch.equal(got, ref):
        bad = got != ref
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} entries differ, max |diff| "
                             f"{float((got - ref).abs().max())}, first at {bad.nonzero()[0].tolist()}")


def _stored_jobs(shapes, N, make, seed):
    """[(dz, inp)] on the CPU for (O, K) shapes"""
    return [(make(N, O, seed + 2 * i), make(N, K, seed + 2 * i + 1)) for i, (O, K) in enumerate(shapes)]


def _launch_exact(pairs, what):
    run = H.run_jobs([(_dev(dz), _dev(inp)) for dz, inp in pairs])
    _good(run, what)
    for i, ((dz, inp), dw) in enumerate(zip(pairs, run.dws)):
        _assert_exact(dw, H.reference(dz, inp), f"{what} job {i} (O {dz.shape[1]}, K {inp.shape[1]})")


@pytest.mark.parametrize("N", [1, 2, 13, 257])
def test_exact_at_every_width_edge(N):
    """6 x 9 widths = 54 shapes, 16 jobs to a launch with the variants mixed."""
    shapes = [(O, K) for K in WIDTHS_K for O in WIDTHS_O]
    shapes = [shapes[(7 * i) % 54] for i in range(54)]            # 7 and 54 are coprime: a permutation
    assert len(set(shapes)) == 54 and {_variant(*s) for s in shapes} == {(o, k) for o in (1, 2) for k in (1, 2, 3)}
    for first in range(0, 54, 16):
        chunk = shapes[first:first + 16]
        assert len({_variant(*s) for s in chunk}) >= 4
        _launch_exact(_stored_jobs(chunk, N, H.int_inputs, first), f"N {N} shapes {first}..")


@pytest.mark.parametrize("N", [1, 2, 3, 11, 12, 13, 23, 24, 25, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 65791,
                               65792, 65793, 131073])
def test_exact_at_every_row_edge(N):
    """One shape per variant, all six in one launch."""
    _launch_exact(_stored_jobs(VARIANTS, N, H.int_inputs, 100), f"N {N}")


@pytest.mark.parametrize("N", [1, 2, 13, 257, 513, 4999])
def test_float_inputs_stay_within_the_rounding_bound(N):
    """The six variants' shapes in one launch, |dw - fp64| <= rounding_bound element by element (observed: the module's
    docstring).  At N <= 13 the bound is about 1e-6 of an entry: an operand rounded to bf16 or xf32 misses it by
    orders of magnitude."""
    from instag_amd import _lib
    pairs = _stored_jobs(VARIANTS, N, H.float_inputs, 200)
    run = H.run_jobs([(_dev(dz), _dev(inp)) for dz, inp in pairs])
    _good(run, f"N {N}")
    ratios = []
    for (dz, inp), dw in zip(pairs, run.dws):
        bound = H.rounding_bound(dz, inp, H.partials(_lib.lib(), N, dz.shape[1], inp.shape[1]))
        ratios.append(float(((dw.cpu().double() - H.reference(dz, inp)).abs() / bound).max()))
    print(f"N {N}: max err / bound per shape {' '.join(f'{r:.4f}' for r in ratios)}")
    for (O, K), r in zip(VARIANTS, ratios):
        assert r <= 1.0, (N, O, K, r)


_FILLER_CACHE = {}


def _fillers(N, make, seed):
    """The 15 stored-row neighbours at N rows, on the device, with their references: made once per (N, kind of data)."""
    key = (N, seed)
    if key not in _FILLER_CACHE:
        _FILLER_CACHE.clear()
        pairs = _stored_jobs(FILLERS, N, make, seed)
        _FILLER_CACHE[key] = ([(_dev(dz), _dev(inp)) for dz, inp in pairs], [H.reference(dz, inp) for dz, inp in pairs])
    return _FILLER_CACHE[key]


def _virtual_inputs(N, split, make, seed):
    KX, KA, KE = split
    cpu = (make(N, 64, seed), make(N, KX, seed + 1), make(N, KA, seed + 2), make(N, KE, seed + 3),
           make(KA, None, seed + 4), make(KE, None, seed + 5))
    return cpu, H.virtual_rows(*cpu[1:])


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("N", [1, 13, 257, 65537])
def test_virtual_rows_exact_in_any_slot(N, split):
    """The glue job (O in {1, 32, 33, 64}) in slot 0, 7 and 15 of a 16-job launch whose other jobs have stored rows:
    equal to the fp64 product with the rows formed in fp32 on the CPU, and every neighbour to its own reference."""
    fill_dev, fill_ref = _fillers(N, H.int_inputs, 300)
    (dz64, inp, aud, eye, enc_a, enc_e), rows = _virtual_inputs(N, split, H.int_inputs, 400)
    if N > 1:
        assert bool((eye < 0).any()) and bool((eye > 0).any())
    ref64 = H.reference(dz64, rows)
    dev = [_dev(t) for t in (inp, aud, eye, enc_a, enc_e)]
    for O in (1, 32, 33, 64):
        dz = _dev(dz64[:, :O].contiguous())
        for slot in (0, 7, 15):
            what = f"N {N} split {split} O {O} slot {slot}"
            run = H.run_jobs(fill_dev[:slot] + [(dz, dev[0])] + fill_dev[slot:], glue=(slot, *dev[1:]))
            _good(run, what)
            assert run.dws[slot].shape == (O, sum(split))
            _assert_exact(run.dws[slot], ref64[:O], what)
            for i, ref in enumerate(fill_ref):
                _assert_exact(run.dws[i if i < slot else i + 1], ref, f"{what} neighbour {FILLERS[i]}")


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_virtual_rows_float_within_the_rounding_bound(split):
    from instag_amd import _lib
    N = 257
    fill_dev, _ = _fillers(N, H.float_inputs, 500)
    (dz64, inp, aud, eye, enc_a, enc_e), rows = _virtual_inputs(N, split, H.float_inputs, 600)
    dev = [_dev(t) for t in (inp, aud, eye, enc_a, enc_e)]
    ratios = []
    for O in (1, 32, 33, 64):
        dz = dz64[:, :O].contiguous()
        run = H.run_jobs(fill_dev[:7] + [(_dev(dz), dev[0])] + fill_dev[7:], glue=(7, *dev[1:]))
        _good(run, f"split {split} O {O}")
        bound = H.rounding_bound(dz, rows, H.partials(_lib.lib(), N, O, sum(split)))
        ratios.append(float(((run.dws[7].cpu().double() - H.reference(dz, rows)).abs() / bound).max()))
    print(f"split {split}: max err / bound per O {' '.join(f'{r:.4f}' for r in ratios)}")
    assert max(ratios) <= 1.0, (split, ratios)


@pytest.mark.parametrize("N", [13, 513])
def test_a_job_is_independent_of_its_launch_and_deterministic(N):
    """Float data, bit for bit: a job alone == through instag_linear_weight_grad == in every slot of a 16-job launch among
    neighbours of other shapes == on a second call."""
    shapes = FILLERS + [(3, 7)]
    jobs = [(_dev(dz), _dev(inp)) for dz, inp in _stored_jobs(shapes, N, H.float_inputs, 700)]
    alone = []
    for i, job in enumerate(jobs):
        run = H.run_jobs([job])
        _good(run, f"N {N} job {i} alone")
        single = H.run_single(*job)
        _good(single, f"N {N} job {i} single entry")
        assert torch.equal(single.dws[0], run.dws[0]), (N, shapes[i], "single-job entry point")
        assert torch.equal(H.run_jobs([job]).dws[0], run.dws[0]), (N, shapes[i], "second call")
        alone.append(run.dws[0].clone())
    for shift in range(16):
        order = [(slot + shift) % 16 for slot in range(16)]
        for attempt in range(2 if shift == 0 else 1):
            run = H.run_jobs([jobs[i] for i in order])
            _good(run, f"N {N} shift {shift}")
            for slot, i in enumerate(order):
                assert torch.equal(run.dws[slot], alone[i]), (N, shapes[i], f"slot {slot}", f"call {attempt}")


def _untouched(run):
    return all(bool(torch.isnan(dw).all()) for dw in run.dws if dw is not None)


def test_workspace_layout_and_one_byte_fewer():
    """The documented byte count (every job rounded up to 256 but the last) suffices, with the canary behind it intact; one
    byte fewer is INSTAG_E_SPACE before anything is launched.  1, 2 and 16 jobs and a glue launch, three partials per
    job, the last job's bytes no multiple of 256."""
    from instag_amd import _lib
    L = _lib.lib()
    N, last = 513, (1, 7)
    aud, eye, enc_a, enc_e = (H.int_inputs(N, 20, 820), H.int_inputs(N, 5, 821), H.int_inputs(20, None, 822),
                              H.int_inputs(5, None, 823))
    virt = tuple(_dev(t) for t in (aud, eye, enc_a, enc_e))
    for shapes, slot in (([last], None), ([(33, 31), last], None), (FILLERS + [last], None), ([(33, 31), (5, 40), last], 1)):
        what = f"{len(shapes)} jobs, glue slot {slot}"
        pairs = _stored_jobs(shapes, N, H.int_inputs, 800)
        jobs = [(_dev(dz), _dev(inp)) for dz, inp in pairs]
        glue = None if slot is None else (slot, *virt)
        rows = [H.virtual_rows(inp, aud, eye, enc_a, enc_e) if i == slot else inp for i, (_, inp) in enumerate(pairs)]
        dims = [(N, dz.shape[1], r.shape[1]) for (dz, _), r in zip(pairs, rows)]
        each = [L.instag_linear_weight_grad_workspace_bytes(*d) for d in dims]
        assert each == [3 * 4 * O * K for _, O, K in dims]
        offsets, total = H.layout(L, dims)
        assert total == sum((b + 255) // 256 * 256 for b in each[:-1]) + each[-1] and total % 256 != 0, what
        assert all(o % 256 == 0 for o in offsets), what
        run = H.run_jobs(jobs, glue=glue, workspace_bytes=total)
        _good(run, what)
        for i, ((dz, _), r, dw) in enumerate(zip(pairs, rows, run.dws)):
            _assert_exact(dw, H.reference(dz, r), f"{what}, job {i}")
        short = H.run_jobs(jobs, glue=glue, workspace_bytes=total - 1)
        assert short.rc == E_SPACE and b"workspace too small" in short.error, (what, short.rc, short.error)
        assert short.intact and _untouched(short), what
        torch.cuda.synchronize()
    dz, inp = jobs[-1]
    _good(H.run_single(dz, inp), "single-job entry point, exact workspace")
    short = H.run_single(dz, inp, workspace_bytes=each[-1] - 1)
    assert short.rc == E_SPACE and b"workspace too small" in short.error, (short.rc, short.error)
    assert short.intact and _untouched(short)


def test_refused_arguments():
    """Nothing is launched for a refused call: a nonzero code, a text, outputs untouched, the device still in order."""
    N = 13
    (dz, inp), (dz2, inp2) = [(_dev(a), _dev(b)) for a, b in _stored_jobs([(33, 31), (5, 40)], N, H.int_inputs, 900)]
    other_n = tuple(_dev(t) for t in _stored_jobs([(33, 31)], N + 1, H.int_inputs, 910)[0])
    cpu, _ = _virtual_inputs(N, (40, 20, 5), H.int_inputs, 920)
    aud, eye, enc_a, enc_e = (_dev(t) for t in cpu[2:])
    aud31, enc31 = _dev(H.int_inputs(N, 31, 930)), _dev(H.int_inputs(31, None, 931))
    eye1, enc1 = _dev(H.int_inputs(N, 1, 932)), _dev(H.int_inputs(1, None, 933))
    inp32 = _dev(H.int_inputs(N, 32, 934))
    ok = (dz, inp)
    virt = (dz2, inp2)                                   # K = 40 + 20 + 5 = 65 as the glue job
    cases = {
        "no jobs": dict(jobs=[]),
        "17 jobs": dict(jobs=[ok] * 17),
        "different N": dict(jobs=[ok, other_n]),
        "N = 0": dict(jobs=[dict(dz=dz, inp=inp, N=0)]),
        "O = 0": dict(jobs=[ok, dict(dz=dz, inp=inp, O=0)]),
        "O = 65": dict(jobs=[dict(dz=dz, inp=inp, O=65), ok]),
        "K = 0": dict(jobs=[ok, dict(dz=dz, inp=inp, K=0)]),
        "K = 97": dict(jobs=[dict(dz=dz, inp=inp, K=97)]),
        "NULL dz": dict(jobs=[ok, dict(dz=None, inp=inp, N=N, O=33)]),
        "NULL inp": dict(jobs=[dict(dz=dz, inp=None, K=31), ok]),
        "NULL dw": dict(jobs=[dict(dz=dz, inp=inp, dw=False)]),
        "glue_job = -1": dict(jobs=[ok, virt], glue=(-1, aud, eye, enc_a, enc_e)),
        "glue_job = n_jobs": dict(jobs=[ok, virt], glue=(2, aud, eye, enc_a, enc_e)),
        "glue job with K = 64": dict(jobs=[ok, (dz2, inp32)], glue=(1, aud31, eye1, enc31, enc1)),
        "glue job with K = 56": dict(jobs=[ok, virt], glue=(0, aud, eye, enc_a, enc_e)),
        "glue job with KA + KE = K": dict(jobs=[ok, dict(dz=dz2, inp=inp2, K=25 + 40)], glue=(1, aud, eye, enc_a, enc_e),
                                          ka_ke=(40, 25)),
        "glue job with KA + KE > K": dict(jobs=[ok, dict(dz=dz2, inp=inp2, K=66)], glue=(1, aud, eye, enc_a, enc_e),
                                          ka_ke=(40, 30)),
        "NULL aud": dict(jobs=[ok, virt], glue=(1, None, eye, enc_a, enc_e)),
    }
    for name, case in cases.items():
        glue = case.get("glue")
        if "ka_ke" in case:             # per-frame vectors of KA and KE entries: KX = K - KA - KE < 1
            KA, KE = case["ka_ke"]
            glue = (glue[0], _dev(H.int_inputs(N, KA, 940)), _dev(H.int_inputs(N, KE, 941)),
                    _dev(H.int_inputs(KA, None, 942)), _dev(H.int_inputs(KE, None, 943)))
        run = H.run_jobs(case["jobs"], glue=glue)
        assert run.rc != 0 and len(run.error) > 0, (name, run.rc, run.error)
        assert run.rc == E_ARG, (name, run.rc, run.error)
        assert run.intact and _untouched(run), name
        torch.cuda.synchronize()
    # ... and the same objects still compute
    _good(H.run_jobs([ok, virt], glue=(1, aud, eye, enc_a, enc_e)), "after the refusals")


def test_mlp_weight_grads_over_more_jobs_than_a_launch_takes():
    """19 jobs over two N, two of them with virtual rows at the same N: _wgrad_launches must split them, and every dw
    comes back in job order, exact on integer data."""
    from instag_amd.mlp import _wgrad_launches, weight_grads
    shapes = FILLERS + [(3, 7)]
    sizes = [257] * 16 + [13]
    cpu_jobs, refs = [], []
    for i, ((O, K), N) in enumerate(zip(shapes + [(5, 9)], sizes)):
        dz, inp = H.int_inputs(N, O, 1000 + 2 * i), H.int_inputs(N, K, 1001 + 2 * i)
        cpu_jobs.append((dz, inp, None))
        refs.append(H.reference(dz, inp))
    for at, split, O in ((0, (36, 32, 6), 64), (1, (31, 33, 31), 33)):
        (dz64, inp, aud, eye, enc_a, enc_e), rows = _virtual_inputs(257, split, H.int_inputs, 1100 + at)
        dz = dz64[:, :O].contiguous()
        cpu_jobs.insert(at, (dz, inp, (aud, eye, enc_a, enc_e)))
        refs.insert(at, H.reference(dz, rows))
    assert len(cpu_jobs) == 19
    jobs = [(_dev(dz), _dev(inp), None if virt is None else tuple(_dev(t) for t in virt)) for dz, inp, virt in cpu_jobs]
    chunks = [list(c) for c in _wgrad_launches(jobs)]
    assert chunks == [[0], list(range(1, 17)), [17], [18]]          # two virtual jobs apart, then 16 to a launch, then N
    assert all(sum(jobs[i][2] is not None for i in c) <= 1 for c in chunks)
    dws = weight_grads(jobs)
    torch.cuda.synchronize()
    assert len(dws) == 19
    for i, (dw, ref) in enumerate(zip(dws, refs)):
        assert bool(torch.isfinite(dw).all()), f"job {i}"
        _assert_exact(dw, ref, f"job {i}")
