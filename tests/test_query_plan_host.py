"""CPU: which kernel every query call runs -- chore_query_plan (csrc/query_plan.h; no handle, no device) against the literal
expectations of query_plan_cases.py, case by case under each of the four switch sets; what the entry points refuse; and the names
bench.py forms for the forward kernel it reports, written out here because bench.py restates the forward rule on its own."""
import ctypes

import pytest

import query_plan_cases as qc


def _plan(op, dtype, B, N, FH, FW, live, flags, switches):
    from chore_amd import _lib
    out = (ctypes.c_int * 9)()
    n = _lib.lib.chore_query_plan(op, dtype, B, N, FH, FW, live, flags, switches, out, 9)
    return n if n < 0 else list(out[:n])


def _name(p):
    """the rocprofv3 name of the plan's kernel (the spelling bench.py and the kernel traces use)"""
    T = {qc.F32: "float", qc.BF16: "unsigned short", qc.F16: "qh16_t"}[p[8]]
    b = lambda bit: "true" if p[3] & bit else "false"  # noqa: E731
    if p[0] == 0:
        return "query_fwd_x3_split_kernel<%s, %d>" % (T, p[1])
    if p[0] == 1:
        return "query_fwd_f32_kernel<%s, %d, %s, %s>" % (T, p[1], b(1), b(4))
    if p[0] == 2:
        return "query_fwd_f32_w8_kernel<%s, %s, %s>" % (T, b(1), b(4))
    return "query_bwd_f32_kernel<%s, %s, %d, %s, %d, %s, %s, %s>" % (T, b(1), p[1], b(2), p[2], b(4), b(8), b(16))


@pytest.mark.parametrize("k", range(len(qc.SWITCH_SETS)), ids=[s[0] for s in qc.SWITCH_SETS])
def test_every_case_runs_the_expected_kernel(k):
    bits = qc.SWITCH_SETS[k][1]
    wrong = []
    for case in qc.CASES:
        name, sort = qc.expected(case, k)
        got = _plan(*case[:8], bits)
        want = qc.plan_of_name(name, sort, case[6])
        if got != want or _name(got) != name:
            wrong.append((case[:8], got, want, name))
    assert not wrong, wrong[:5]


def test_case_list_covers_the_rules():
    """every instantiation family, both tile sizes, the sort and every switch appear in the expectations"""
    names = {qc.expected(c, k) for c in qc.CASES for k in range(4)}
    kernels = {n for n, _ in names}
    assert len(kernels) >= 40 and any(s for _, s in names)
    for k in (1, 2, 3):         # each switch changes some case
        assert any(qc.expected(c, k) != qc.expected(c, 0) for c in qc.CASES), qc.SWITCH_SETS[k][0]


def test_refused_combinations():
    for op, dtype, flags in qc.REFUSED:
        for _, bits, _ in qc.SWITCH_SETS:
            assert _plan(op, dtype, 4, 4097, 16, 16, 15, flags, bits) == qc.EINVAL, (op, dtype, flags)
    # bad arguments: the operation, the dtype, the shape
    for a in ((5, qc.F32, 4, 64, 16, 16), (-1, qc.F32, 4, 64, 16, 16), (qc.FWD, 7, 4, 64, 16, 16), (qc.FWD, qc.F32, 0, 64, 16, 16),
              (qc.FWD, qc.F32, 4, 0, 16, 16), (qc.FWD, qc.F32, 4, 64, 1, 16)):
        assert _plan(*a, 0, 0, 0) == qc.EINVAL, a


def test_environment_is_the_default_switch_set(monkeypatch):
    """switches = -1: this process's environment, which sets none of the three switches under pytest"""
    import os
    assert not any(os.environ.get(v) for _, _, env in qc.SWITCH_SETS for v in env)
    for case in qc.CASES[::7]:
        assert _plan(*case[:8], -1) == _plan(*case[:8], 0)


def test_forward_names_bench_reports():
    """bench.py (the lines that form `qname`) names the forward kernel of its step from B, N and the dtype mode; these are those names
    for its four modes at its own shape and at a small one, with and without CHORE_QUERY_X3_NOSPLIT -- the one switch it reads"""
    modes = {"fp32": qc.F32, "fp16x3": qc.F16X3, "bf16": qc.BF16 | qc.X3, "fp16": qc.F16}
    want = {
        ("fp32", 20000, 0): "query_fwd_f32_w8_kernel<float, false, false>",
        ("fp32", 333, 0): "query_fwd_f32_kernel<float, 1, false, false>",
        ("fp16x3", 20000, 0): "query_fwd_x3_split_kernel<float, 2>",
        ("fp16x3", 333, 0): "query_fwd_x3_split_kernel<float, 1>",
        ("bf16", 20000, 0): "query_fwd_x3_split_kernel<unsigned short, 2>",
        ("bf16", 333, 0): "query_fwd_x3_split_kernel<unsigned short, 1>",
        ("fp16", 20000, 0): "query_fwd_x3_split_kernel<qh16_t, 2>",
        ("fp16", 333, 0): "query_fwd_x3_split_kernel<qh16_t, 1>",
        ("fp32", 20000, 2): "query_fwd_f32_w8_kernel<float, false, false>",
        ("fp32", 333, 2): "query_fwd_f32_kernel<float, 1, false, false>",
        ("fp16x3", 20000, 2): "query_fwd_f32_kernel<float, 2, false, true>",
        ("fp16x3", 333, 2): "query_fwd_f32_kernel<float, 1, false, true>",
        ("bf16", 20000, 2): "query_fwd_f32_kernel<unsigned short, 2, false, true>",
        ("bf16", 333, 2): "query_fwd_f32_kernel<unsigned short, 1, false, true>",
        ("fp16", 20000, 2): "query_fwd_f32_kernel<qh16_t, 2, false, true>",
        ("fp16", 333, 2): "query_fwd_f32_kernel<qh16_t, 1, false, true>",
    }
    for (mode, N, bits), name in want.items():
        B = 4 if N == 20000 else 2
        assert _name(_plan(qc.FWD, modes[mode], B, N, 128, 128, 0, 0, bits)) == name, (mode, N, bits)
