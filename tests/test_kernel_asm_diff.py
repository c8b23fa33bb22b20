"""tools/kernel_asm_diff.py on small hand-written assembly: a kernel that moved to another file
position (its local labels renumbered) is identical; a changed instruction, a changed register
count, a new kernel and a missing kernel that is not on the removal list are each reported."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "kernel_asm_diff.py")


def kernel(name, f, add="v_add_f32_e32 v0, v0, v1", vgpr=4):
    return """
	.globl	{n}
	.p2align	8
	.type	{n},@function
{n}:                                  ; @{n}
; %bb.0:
	s_load_dwordx2 s[0:1], s[0:1], 0x0
	s_cbranch_scc1 .LBB{f}_2
; %bb.1:                                ; some comment
	{add}
.LBB{f}_2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {n}
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr {v}
	.end_amdhsa_kernel
	.text
.Lfunc_end{f}:
	.size	{n}, .Lfunc_end{f}-{n}
                                        ; -- End function
	.set {n}.num_vgpr, {v}
	.set {n}.private_seg_size, 0
""".format(n=name, f=f, add=add, v=vgpr)


def run(tmp_path, old, new, removed=None, exact=False):
    paths = {}
    for side, texts in (("old", old), ("new", new)):
        paths[side] = []
        for i, t in enumerate(texts):
            p = tmp_path / ("%s%d.s" % (side, i))
            p.write_text(t)
            paths[side].append(str(p))
    cmd = [sys.executable, TOOL, "--old"] + paths["old"] + ["--new"] + paths["new"]
    if removed is not None:
        r = tmp_path / "removed.txt"
        r.write_text(removed)
        cmd += ["--removed", str(r)] + (["--exact"] if exact else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    return res.returncode, res.stdout


def test_moved_kernels_are_identical(tmp_path):
    old = [kernel("ka", 0) + kernel("kb", 1) + kernel("kc", 2)]
    new = [kernel("kc", 0), kernel("ka", 5)]  # two files, other function indices; kb is gone
    rc, out = run(tmp_path, old, new, removed="# gone on purpose\nkb$\n", exact=True)
    assert rc == 0, out
    assert "identical: 2   differing: 0   only in new: 0   only in old: 1" in out
    rc, out = run(tmp_path, old, new, removed="nothing_matches\n")
    assert rc == 1 and "NOT ON THE REMOVAL LIST: kb" in out
    rc, out = run(tmp_path, old, new, removed="kb$\nkz$\n", exact=True)
    assert rc == 1 and "MATCHES NOTHING: kz$" in out


def test_differences_are_reported(tmp_path):
    old = [kernel("ka", 0) + kernel("kb", 1)]
    rc, out = run(tmp_path, old, [kernel("ka", 0, add="v_mul_f32_e32 v0, v0, v1") + kernel("kb", 1)])
    assert rc == 1 and "DIFFERS: ka" in out and "instructions" in out
    rc, out = run(tmp_path, old, [kernel("ka", 0) + kernel("kb", 1, vgpr=8)])
    assert rc == 1 and "DIFFERS: kb" in out and "resources" in out
    rc, out = run(tmp_path, old, [kernel("ka", 0) + kernel("kb", 1) + kernel("kn", 2)])
    assert rc == 1 and "ONLY IN NEW: kn" in out
    rc, out = run(tmp_path, old, [kernel("ka", 0), kernel("ka", 3, vgpr=8) + kernel("kb", 1)])
    assert rc == 1 and "DIFFERS BETWEEN THE NEW FILES: ka" in out
