"""CPU: the coverage table of tests/test_gpu_fit_kernels.py (fit_cases.COVERAGE) names every entry point of the fitting-step and
evaluation families of chore_amd/_lib.py, every case family is run by a GPU test, and the constants the shapes were chosen around
are the ones in the .hip sources: a new entry point without a row, a family without a test or a changed tile size fails here,
before anyone reaches a GPU.  Also here, because they need no GPU: the float64 LBS restatement of tests/fit_ref.py against the
reference layer's outputs (tests/golden/smpl_lbs.npz), and the cap on the nearest-neighbour ties of the contact cases."""
import os
import re

import numpy as np
import torch

import fit_cases as fc
import fit_ref as fr
from conftest import REPO, golden

CSRC = os.path.join(REPO, "chore_amd", "csrc")


def _src(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_table_names_exactly_the_entry_points():
    text = open(os.path.join(REPO, "chore_amd", "_lib.py")).read()
    names = set(re.findall(r'^\s*"(chore_\w+)"\s*:\s*\(', text, re.M))
    want = {n for n in names if n.startswith(fc.FAMILIES)}
    assert len(want) == 31, sorted(want)
    assert set(fc.COVERAGE) == want, (sorted(want - set(fc.COVERAGE)), sorted(set(fc.COVERAGE) - want))
    # ... and the header declares the same ones
    header = open(os.path.join(REPO, "include", "chore_hip.h")).read()
    declared = {n for n in re.findall(r"\b(chore_\w+)\(", header) if n.startswith(fc.FAMILIES)}
    assert declared == want, sorted(declared ^ want)


def test_rows_are_case_ids_or_reasons():
    every = {c["id"] for cs in fc.CASES.values() for c in cs}
    assert len(every) == sum(len(cs) for cs in fc.CASES.values()), "duplicate case ids"
    used = set()
    print("coverage table (%d rows):" % len(fc.COVERAGE))
    for name, row in fc.COVERAGE.items():
        if isinstance(row, str):
            assert len(row) > 20, name
            print("  %-40s not covered here: %s" % (name, row))
        else:
            assert row and set(row) <= every, name
            used |= set(row)
            print("  %-40s %d cases" % (name, len(row)))
    assert used == every, sorted(every - used)         # no case that reaches no entry point of the table
    # the three landmark cases that exist stay where they are
    smpl = open(os.path.join(REPO, "tests", "test_gpu_smpl.py")).read()
    assert "def test_landmark_regression_forward_and_backward(B)" in smpl and '@pytest.mark.parametrize("B", [1, 3])' in smpl
    assert "def test_rot_noise_operator()" in open(os.path.join(REPO, "tests", "test_gpu_fit.py")).read()


def test_every_case_family_is_run_by_a_gpu_test():
    text = open(os.path.join(REPO, "tests", "test_gpu_fit_kernels.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    run = re.findall(r'@pytest\.mark\.parametrize\("case", fc\.CASES\["(\w+)"\], ids=fc\.ids\("(\w+)"\)\)\ndef (test_\w+)\(case\):', text)
    assert all(a == b for a, b, _ in run), run
    assert sorted(a for a, _, _ in run) == sorted(fc.CASES), (run, sorted(fc.CASES))


def test_the_matrix_holds_the_shapes_it_was_asked_for():
    C = fc.CASES
    vals = lambda fam, key: {c[key] for c in C[fam]}       # noqa: E731
    # no case may leave quietly: the size of every family, and the full products where the matrix is one
    assert {k: len(v) for k, v in C.items()} == {"lbs": 34, "smpl_terms": 16, "point_terms": 39, "obj_transform": 8, "obj_terms": 10, "so3": 11,
                                                 "contact": 36, "adam": 15, "step": 5, "chamfer": 5, "procrustes": 7}
    assert len({(c["B"], c["offsets"], c["up"]) for c in C["lbs"] if c["pose"] == "random"}) == 5 * 2 * 3
    assert len({(c["B"], c["R"]) for c in C["smpl_terms"]}) == 3 * 3
    assert len({(c["N"], c["B"], c["C"]) for c in C["point_terms"] if c["C"]}) == 5 * 2 * 3
    assert len({(c["Nh"], c["No"], c["P"], c["B"]) for c in C["contact"] if c["null"] is None and c["frames"] in ("plain", "mixed")}) == 5 * 3 * 2
    assert len({(c["n"], c["nt"]) for c in C["adam"] if not (c["frozen"] or c["slices"] or c["acc_only"])}) == 5 * 2
    for fam in ("obj_transform", "obj_terms"):
        assert len({(c["N"], c["B"]) for c in C[fam]}) == 4 * 2
    assert vals("lbs", "B") == {1, 3, 4, 5, 9} and vals("lbs", "offsets") == {0, 1} and vals("lbs", "up") == {"verts", "joints", "both"}
    assert vals("lbs", "pose") == {"random", "zero", "tiny", "near_pi", "zero_betas"}
    assert any(c["B"] % fc.CONSTANTS["FB"] == 1 and c["B"] > fc.CONSTANTS["FB"] for c in C["lbs"])      # a last group of one frame
    assert vals("smpl_terms", "B") == {1, 3, 8} and vals("smpl_terms", "R") == {25, 137, 256}
    assert vals("smpl_terms", "null_up") == {None, 0, 1, 2, 3, 4} and vals("smpl_terms", "kpts") == {True, False}
    assert any(c["conf_zero"] for c in C["smpl_terms"])
    assert {(r["P"], r["R"]) for r in fc.SMPL_TERMS_REFUSED} >= {(156, 24), (156, 257), (72, 137)}
    blk = fc.CONSTANTS["PT_BLOCK"]
    assert vals("point_terms", "N") == {1, blk - 1, blk, blk + 1, 1000} and vals("point_terms", "B") == {1, 3}
    assert vals("point_terms", "C") == {0, 1, 14, fc.CONSTANTS["PT_MAXC"]} and vals("point_terms", "channel") == {0, 1}
    assert vals("point_terms", "logits") == {None, "normal", "pm80"} and vals("point_terms", "null_up") == {None, 0, 1}
    for fam in ("obj_transform", "obj_terms"):
        assert vals(fam, "N") == {1, blk - 1, blk + 1, 3000} and vals(fam, "B") == {1, 3}
    assert vals("obj_terms", "null_up") == {None, 0, 1}
    per = fc.CONSTANTS["SO3_PER_BLOCK"]
    assert vals("so3", "B") == {1, per, per + 1, 2 * per + 2}
    assert {n for c in C["so3"] for n in c["content"]} == set(fc.SO3_CONTENT)
    t = fc.CONSTANTS["TILE"]
    assert {(c["Nh"], c["No"]) for c in C["contact"]} == {(1, 1), (t - 1, t + 1), (t, t), (2 * t + 1, 40), (700, 300)}
    assert vals("contact", "P") == {1, 14, fc.CONSTANTS["CP_MAX"]} and vals("contact", "B") == {1, 3} and fc.CONTACT_REFUSED_P == fc.CONSTANTS["CP_MAX"] + 1
    assert vals("contact", "null") == {None, "hum", "obj"}
    assert vals("contact", "frames") == {"plain", "mixed", "none", "obj_none", "one_sided_part", "single_pair"}
    cap = fc.CONSTANTS["ADAM_BLOCK"] * fc.CONSTANTS["ADAM_MAX_BLOCKS"]
    assert vals("adam", "n") >= {1, 255, 257, cap + 1, 40000} and 40000 > 2 * cap and vals("adam", "nt") == {1, fc.CONSTANTS["FS_MAXT"]}
    assert vals("adam", "api") == {"step", "acc"} and vals("adam", "frozen") == {True, False} and vals("adam", "counted") == {0, 1}
    assert any(c["slices"] for c in C["adam"]) and any(c["acc_only"] for c in C["adam"]) and fc.ADAM_STEPS == 3
    assert any(acc for c in C["adam"] for _, _, _, acc in fc.adam_layout(c)) and any(cols < n for c in C["adam"] for n, cols, _, _ in fc.adam_layout(c))
    assert {c.get("n") for c in C["step"]} == {None, 1, fc.CONSTANTS["FS_MAXL"]} and len(fc.RULE_TABLE) == len(set(fc.RULE_TABLE)) == 8
    nt, nb = fc.CONSTANTS["NN_TILE"], fc.CONSTANTS["NN_BLOCK"]
    assert {(c["Nx"], c["Ny"]) for c in C["chamfer"] if not c["dup"]} == {(1, 1), (nb - 1, nt + 1), (nt, nt), (2 * nt + 1, 300)}
    assert any(c["dup"] for c in C["chamfer"])
    assert vals("procrustes", "N") == {3, 255, 257, 1500} and vals("procrustes", "kind") == {"generic", "planar", "reflected", "offset"}


def test_constants_are_the_sources():
    K = fc.CONSTANTS
    const = lambda src, name: int(re.search(r"constexpr int (?:\w+ = \d+, )*%s = (\d+)" % name, src).group(1))      # noqa: E731
    lbs = _src("smpl_lbs.hip")
    assert const(lbs, "FB") == K["FB"] and const(lbs, "VF_V") == K["VF_V"]
    assert "const int b0 = blockIdx.y * FB, nf = min(FB, B - b0);" in lbs and "const int b0 = grp * FB, nf = min(FB, B - b0), tid = threadIdx.x;" in lbs
    assert "else if (y < (B + FB - 1) / FB) lbs_dpm_body(" in lbs and "gv[f] = work + wk.gvp + (size_t)(b0 + min(f, nf - 1)) * V3;" in lbs
    assert "lbs_vertex_bwd_kernel, dim3((V + 255) / 256, B), dim3(256)" in lbs and K["LBS_BWD_BLOCK"] == 256
    assert fc.V_SMPL % K["VF_V"] and fc.V_SMPL % K["LBS_BWD_BLOCK"]            # the last workgroup of both vertex kernels is ragged
    con = _src("contact.hip")
    assert const(con, "TILE") == K["TILE"] and const(con, "CP_MAX") == K["CP_MAX"]
    ft = _src("fit_terms.hip")
    assert const(ft, "PT_MAXC") == K["PT_MAXC"]
    assert len(re.findall(r"dim3\(\(N \+ 255\) / 256, B\), dim3\(256\)", ft)) == 3 and ft.count("dim3(chunks, B), dim3(256)") == 1 and K["PT_BLOCK"] == 256
    assert "const int chunks = (N + 255) / 256;" in ft
    fs = _src("fit_step.hip")
    assert const(fs, "FS_MAXT") == K["FS_MAXT"] and const(fs, "FS_MAXL") == K["FS_MAXL"]
    m = re.search(r"int bx = \(nmax \+ (\d+)\) / (\d+);\s*if \(bx > (\d+)\) bx = (\d+);", fs)
    assert m and (int(m.group(1)) + 1, int(m.group(2))) == (K["ADAM_BLOCK"], K["ADAM_BLOCK"]) and int(m.group(3)) == int(m.group(4)) == K["ADAM_MAX_BLOCKS"]
    assert "fit_adam_kernel, dim3(bx, nt), dim3(256)" in fs
    ev = _src("eval_metrics.hip")
    assert const(ev, "NN_TILE") == K["NN_TILE"]
    assert ev.count("nn_min_kernel, dim3((Nx + 255) / 256), dim3(256)") == 1 and ev.count("nn_min_kernel, dim3((Ny + 255) / 256), dim3(256)") == 1
    assert K["NN_BLOCK"] == 256
    so3 = _src("so3.hip")
    assert len(re.findall(r"dim3\(\(B \+ 63\) / 64\), dim3\(64\)", so3)) == 2 and K["SO3_PER_BLOCK"] == 64
    # the contract both files state for inputs of rank <= 1
    for name in ("so3.hip", "svd3.h"):
        assert "rank <= 1" in open(os.path.join(CSRC, name)).read(), name


def test_lbs_restatement_reproduces_the_reference_layer():
    """positions to 1e-6 against the reference SMPL_Layer's float32 outputs, in float64 and in the float32 of the reference itself"""
    from test_oracle_smpl import smpl_inputs
    g, model, offs = smpl_inputs()
    sel = g["sel"]
    for dtype in (torch.float64, torch.float32):
        m = fr.lbs_model(model, dtype)
        c = lambda a: torch.as_tensor(a, dtype=dtype)      # noqa: E731
        v, j, vp, nk = (a.double().numpy() for a in fr.lbs(m, c(g["pose"]), c(g["betas"]), c(g["trans"]), c(offs)))
        errs = [np.abs(v[:, sel] - g["verts_sel"]).max(), np.abs(j - g["joints"]).max(), np.abs(vp[:, sel] - g["v_posed_sel"]).max(),
                np.abs(nk[:, sel] - g["naked_sel"]).max()]
        print("  %s: verts %.2e joints %.2e v_posed %.2e naked %.2e" % ((dtype,) + tuple(errs)))
        assert max(errs) <= 1e-6, (dtype, errs)
        assert np.abs(np.abs(v).sum(1) - g["verts_abs"]).max() <= 2e-5 * np.abs(g["verts_abs"]).max()
    # the gradients of the golden file (the reference layer's own autograd, float32): the float64 restatement within the 2e-4 of
    # tests/test_gpu_smpl.py
    rs = np.random.RandomState(int(g["w_verts_seed"]))
    rs.standard_normal((2, 6890, 3))
    wv = rs.standard_normal((2, 6890, 3)).astype(np.float32)
    out = fr.lbs_with_grads(fr.lbs_model(model), g["pose"], g["betas"], g["trans"], offs, 1.0, wv, g["w_joints"])
    for got, name in zip(out[4:], ("dpose", "dbetas", "dtrans")):
        assert np.abs(got - g[name]).max() <= 2e-4 * np.abs(g[name]).max(), name


def test_contact_ties_stay_within_their_cap():
    """on the reference alone: the points left out of the gradient comparison of a contact case (nearest and second-nearest
    neighbour closer than 1e-6 relative) are at most 0.5 % of the points that take part; and no distance sits within 1e-6 of the
    threshold, no two logits of a point tie"""
    total = 0
    for c in fc.CASES["contact"]:
        hum, obj, df_h, df_o, labels, logits, g = fc.contact_inputs(c)
        assert labels.min() >= 0 and labels.max() < c["P"]
        for df in (df_h, df_o):
            assert (np.abs(df.astype(np.float64) - float(np.float32(fc.THRES))) > 1e-6).all(), c["id"]
        top2 = np.sort(logits, 1)[:, -2:]
        assert c["P"] == 1 or (top2[:, 1] > top2[:, 0]).all(), c["id"]
        loss, dh, do, tie_h, tie_o, npart = fr.contact(hum, obj, df_h, df_o, labels, logits, c["P"], float(np.float32(fc.THRES)), float(g))
        ties = int(tie_h.sum() + tie_o.sum())
        total += ties
        assert ties <= fc.CONTACT_TIE_CAP * npart, (c["id"], ties, npart)
        if c["frames"] == "none":
            assert npart == 0 and loss == 0.0
        elif c["frames"] in ("plain", "mixed") and c["P"] == 1:
            assert npart > 0 and loss > 0.0, c["id"]
    print("  contact cases: %d points on a nearest-neighbour tie in all" % total)
