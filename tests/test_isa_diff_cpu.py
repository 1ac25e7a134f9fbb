"""tools/isa_diff.py on small assemblies written here: what it calls identical, what it reports, its exit status.

The mangled names are real ones (c++filt demangles them): _Z3k_aILi1EEvPf is `void k_a<1>(float*)`,
_Z3k_aILi1ELb0EEvPfS0_ is `void k_a<1, false>(float*, float*)`, _Z3k_bPf is `k_b(float*)`."""
from tools import isa_diff


def _kernel(name, body, idx=0, vgpr=12, lds=0):
    text = f"""\t.text
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                ; @{name}
; %bb.0:
{body}\ts_endpgm
.Lfunc_end{idx}:
\t.size\t{name}, .Lfunc_end{idx}-{name}
"""
    meta = f"""  - .args:
      - .address_space:  global
        .name:           out
        .offset:         0
    .group_segment_fixed_size: {lds}
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .symbol:         {name}.kd
    .vgpr_count:     {vgpr}
"""
    return text, meta


def _asm(*kernels):
    return ("".join(k[0] for k in kernels) + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(k[1] for k in kernels) +
            "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


def _loop(label, operand="v1"):
    return f"""\tv_mov_b32_e32 v0, 0                  ; a comment
.{label}:                                ; =>This Inner Loop Header: Depth=1
\t.loc\t1 12 3
\tv_add_f32_e32 v0, v0, {operand}
\ts_cbranch_scc1 .{label}
"""


KA, KA2, KB = "_Z3k_aILi1EEvPf", "_Z3k_aILi1ELb0EEvPfS0_", "_Z3k_bPf"


def _run(tmp_path, capsys, parent, change, *args):
    (tmp_path / "p.s").write_text(parent)
    (tmp_path / "c.s").write_text(change)
    rc = isa_diff.main([str(tmp_path / "p.s"), str(tmp_path / "c.s"), *args])
    return rc, capsys.readouterr().out


def test_renumbered_labels_compare_equal(tmp_path, capsys):
    # the change has another function in front, so k_a's labels carry other numbers; comments and .loc differ too
    parent = _asm(_kernel(KA, _loop("LBB0_1")), _kernel(KB, _loop("LBB1_1"), 1))
    change = _asm(_kernel(KB, _loop("LBB0_3"), 0), _kernel(KA, _loop("LBB1_7").replace("a comment", "another"), 1))
    rc, out = _run(tmp_path, capsys, parent, change)
    assert rc == 0, out
    assert out.count("identical") == 3 and "2 of 2 functions identical" in out  # two lines and the summary
    assert "k_a<1>: 12 / 12, 10 / 10, 0 / 0, 0 / 0" in out


def test_one_changed_operand_is_reported(tmp_path, capsys):
    parent = _asm(_kernel(KA, _loop("LBB0_1")), _kernel(KB, _loop("LBB1_1"), 1))
    change = _asm(_kernel(KA, _loop("LBB0_1", operand="v2")), _kernel(KB, _loop("LBB1_1"), 1))
    rc, out = _run(tmp_path, capsys, parent, change)
    assert rc == 1
    line = next(ln for ln in out.splitlines() if ln.startswith("DIFFERS"))
    assert "k_a<1>" in line and "v_add_f32_e32 v0, v0, v1" in line and "v_add_f32_e32 v0, v0, v2" in line
    assert any(ln.startswith("identical") and "k_b" in ln for ln in out.splitlines())
    assert "1 of 2 functions identical, 1 differ" in out


def test_a_branch_to_another_label_is_a_difference(tmp_path, capsys):
    two = "\ts_nop 0\n.LBB0_1:\n\ts_nop 1\n.LBB0_2:\n\ts_cbranch_scc1 .LBB0_1\n"
    rc, out = _run(tmp_path, capsys, _asm(_kernel(KB, two)), _asm(_kernel(KB, two.replace("scc1 .LBB0_1", "scc1 .LBB0_2"))))
    assert rc == 1 and "DIFFERS" in out


def test_kernel_on_one_side_only_is_reported(tmp_path, capsys):
    both = _asm(_kernel(KA, _loop("LBB0_1")), _kernel(KB, _loop("LBB1_1"), 1))
    one = _asm(_kernel(KA, _loop("LBB0_1")))
    rc, out = _run(tmp_path, capsys, both, one)
    assert rc == 1 and "NO PARTNER  k_b  (only in parent)" in out
    rc, out = _run(tmp_path, capsys, one, both)
    assert rc == 1 and "NO PARTNER  k_b  (only in change)" in out


def test_pair_matches_renamed_kernels(tmp_path, capsys):
    parent = _asm(_kernel(KA, _loop("LBB0_1")))
    change = _asm(_kernel(KA2, _loop("LBB0_1")))
    rc, out = _run(tmp_path, capsys, parent, change)
    assert rc == 1 and out.count("NO PARTNER") == 2
    rc, out = _run(tmp_path, capsys, parent, change, "--pair", "k_a<1>=k_a<1, false>")
    assert rc == 0, out
    assert "identical   k_a<1, false>" in out and "1 of 1 functions identical" in out


def test_unequal_resources_are_flagged(tmp_path, capsys):
    parent = _asm(_kernel(KB, _loop("LBB0_1"), vgpr=12, lds=1024))
    change = _asm(_kernel(KB, _loop("LBB0_1"), vgpr=16, lds=2048))
    rc, out = _run(tmp_path, capsys, parent, change)
    assert rc == 1 and "identical   k_b" in out
    assert "k_b: 12 / 16, 10 / 10, 0 / 0, 1024 / 2048   <-- UNEQUAL" in out
