"""CPU: the coverage table of tests/test_gpu_wgrad_kernels.py (wgrad_cases.COVERAGE) names every weight-gradient instantiation that
conv2d_bwd_weight_impl and chore_gemm_tn_f32 (csrc/train_bwd.hip) can launch.  The launches are parsed out of the source: a new
instantiation without a row in the table -- hence without a matrix case, or without a written reason -- fails here, before anyone
reaches a GPU."""
import os
import re

import wgrad_cases as wc
from conftest import REPO

SRC = os.path.join(REPO, "chore_amd", "csrc", "train_bwd.hip")
NAMES = {"wgrad_kernel": "w32", "wgrad64_kernel": "w64", "wgrad64_x3_kernel": "w64x3", "wgrad64_x3_pc_kernel": "w64x3pc",
         "wgrad128_x3_pc_kernel": "w128x3pc"}
ELEMENT = {"w64": "bf16", "w64x3": "x3", "w64x3pc": "x3", "w128x3pc": "x3"}


def _body(src, head):
    """the text of the function whose definition starts with `head`, up to the first closing brace in column 0"""
    i = src.index(head)
    return src[i:src.index("\n}", i)]


def _launches(body):
    """(kernel, element type, taps) of every CHORE_LAUNCH of a wgrad..._kernel in `body`"""
    out = []
    for m in re.finditer(r"CHORE_LAUNCH\(h, s, \(?(wgrad\w*_kernel)(?:<([^>]*)>)?\)?,", body):
        kern, args = NAMES[m.group(1)], [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
        if kern == "w32":
            assert len(args) == 2, m.group(0)
            out.append((kern, {"float": "fp32", "bf16_t": "bf16"}[args[0]], int(args[1])))
        elif kern == "w128x3pc":
            assert not args, m.group(0)
            out.append((kern, "x3", 1))
        else:
            assert len(args) == 1, m.group(0)
            out.append((kern, ELEMENT[kern], int(args[0])))
    return out


def _src():
    return re.sub(r"//[^\n]*", "", open(SRC).read())


def test_table_names_every_launched_instantiation():
    src = _src()
    got = _launches(_body(src, "int conv2d_bwd_weight_impl("))
    assert len(got) == len(set(got)) == 11, got
    assert sorted(got) == sorted(wc.INSTANTIATIONS), got
    for kern, dt, taps in got:
        for mapping in (("grid",) if kern == "w32" else ("xcd", "linear")):
            # every one ships, under both mappings: each must be reached, not explained away
            assert wc.COVERAGE.get((kern, dt, taps, mapping), "") is None, (kern, dt, taps, mapping)
    assert _launches(_body(src, "int chore_gemm_tn_f32(")) == [("w32", "fp32", 1)]
    assert len(wc.COVERAGE[("w32", "fp32", 1, "gemm_tn")]) > 20
    # nothing else in the file launches one of these kernels, and every kernel template of the file is known here
    assert len(re.findall(r"CHORE_LAUNCH\(h, s, \(?wgrad", src)) == 12
    assert not re.search(r"hipLaunchKernelGGL\(\(?wgrad(?!_finish)", src)
    assert set(re.findall(r"void (wgrad\w*_kernel)\(WgradArgs a\)", src)) == set(NAMES)


def test_mapping_rule_and_witness_codes_are_the_sources():
    src = _src()
    # the two block -> (share, pair) mappings of the 64- and 128-channel kernels, chosen by S % 8 as the witness flag says: one
    # predicate, one mapping helper that applies it, and the witness flag computed through the same predicate
    assert len(re.findall(r"\bwgrad_xcd_mapping\(int S\)", src)) == 1
    assert "__host__ __device__ inline bool wgrad_xcd_mapping(int S) { return S % 8 == 0; }" in src
    assert src.count("S % 8 == 0") == 1
    helper = _body(src, "__device__ __forceinline__ void wgrad_share_pair(")
    assert src.count("const int xcd = L & 7") == 1 and "if (wgrad_xcd_mapping(S)) { const int xcd = L & 7" in helper
    assert helper.count("blockIdx.x") == 1
    for kern in NAMES:
        body = _body(src, "void %s(WgradArgs a)" % kern)
        if kern == "wgrad_kernel":
            assert "wgrad_share_pair" not in body and "wgrad_xcd_mapping" not in body
        else:
            assert body.count("wgrad_share_pair(a.S, npairs, share, pair);") == body.count("wgrad_share_pair") == 1, kern
            assert "blockIdx.x" not in body and "wgrad_xcd_mapping" not in body, kern
    assert "p.ct >= 64 && wgrad_xcd_mapping(p.S) ? WGRAD_FLAG_XCD : 0" in _body(src, "int conv2d_bwd_weight_impl(")
    common = open(os.path.join(REPO, "chore_amd", "csrc", "common.h")).read()
    m = re.search(r"enum \{ WGRAD_K_W32 = (\d), WGRAD_K_W64 = (\d), WGRAD_K_W64X3 = (\d), WGRAD_K_W64X3PC = (\d), WGRAD_K_W128X3PC = (\d) \};", common)
    assert m and {int(v): k for v, k in zip(m.groups(), ("w32", "w64", "w64x3", "w64x3pc", "w128x3pc"))} == wc.KERNELS
    m = re.search(r"enum \{ WGRAD_FLAG_GN = (\d), WGRAD_FLAG_DBIAS = (\d), WGRAD_FLAG_XCD = (\d) \};", common)
    assert m and tuple(int(v) for v in m.groups()) == (wc.FLAG_GN, wc.FLAG_DBIAS, wc.FLAG_XCD)


def test_table_rows_are_reached_or_explained():
    for k, why in wc.COVERAGE.items():
        assert why is None or len(why) > 20, k
    print("coverage table (%d rows, %d to reach):" % (len(wc.COVERAGE), sum(w is None for w in wc.COVERAGE.values())))
    for k, why in wc.COVERAGE.items():
        print("  %-36s %s" % (k, "to reach" if why is None else "not covered: " + why))
    # every case of the matrix runs in at least one switch set, and every switch set has cases
    ran = set()
    for name in wc.SWITCH_SETS:
        jobs = wc.jobs_of(name)
        assert jobs, name
        ran |= {c["id"] for c, _ in jobs}
    assert ran == {c["id"] for c in wc.cases()}
    # every shape runs with GroupNorm recomputed and without, some with dbias, and the poisoned run has its shapes
    assert {c["kind"] for c in wc.cases()} == set(wc.KINDS)
    assert 0 < sum(s["bias"] for s in wc.SHAPES) < len(wc.SHAPES) and any(s["poison"] for s in wc.SHAPES)
    # the x3 gradient scales span 1e-7 ... 3e4
    used = {c["x3_scale"] for c in wc.cases() if wc.uses64(c)}
    assert min(used) == 1e-7 and max(used) == 3e4
