"""tools/kernel_isa_diff.py on small synthetic device assembly (CPU only).

The tool judges whether a change left every kernel's instructions alone, with one side possibly the concatenation
of several units' assembly.  Checked here: label comments that differ only in padding compare equal, a changed
instruction and a kernel of one side only fail, a kernel that occurs twice on one side fails, and --rename pairs
a kernel with its renamed successor.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def kernel(name, ordinal, body=("v_add_u32_e32 v1, v0, v0",), pad="    ", vgprs=8):
    """One kernel as the compiler prints it: symbol, blocks with comments, function-end label, resource summary."""
    insns = "".join(f"\t{i}\n" for i in body)
    return (f"\t.globl\t{name}\n{name}:                            ; @{name}\n"
            f"; %bb.0:\n"
            f"\ts_load_dword s0, s[4:5], 0x0\n"
            f".LBB{ordinal}_1:{pad}; =>This Inner Loop Header: Depth=1\n"
            f"{insns}"
            f"\ts_cbranch_scc1 .LBB{ordinal}_1       ; encoding: [0x00]\n"
            f"; %bb.2:\n"
            f"\ts_endpgm\n"
            f".Lfunc_end{ordinal}:\n"
            f"\t.size\t{name}, .Lfunc_end{ordinal}-{name}\n"
            f"; Kernel info:\n; codeLenInByte = 24\n; TotalNumSgprs: 10\n; NumVgprs: {vgprs}\n; NumAgprs: 0\n"
            f"; ScratchSize: 0\n; LDSByteSize: 0 bytes/workgroup (compile time only)\n")


def run(tmp_path, monkeypatch, capsys, old, new, *args):
    a, b, j = tmp_path / "a.s", tmp_path / "b.s", tmp_path / "out.json"
    a.write_text(old)
    b.write_text(new)
    monkeypatch.setattr("sys.argv", ["kernel_isa_diff.py", str(a), str(b), "--json", str(j), *args])
    try:
        status = isa_diff.main()
    except SystemExit as e:  # a refusal: message on stderr, or as the exit value
        status = e.code
    out = capsys.readouterr()
    rep = json.loads(j.read_text())["kernels"] if j.exists() else None
    return status, out.out + out.err + (status if isinstance(status, str) else ""), rep


def test_label_comment_padding_is_not_a_difference(tmp_path, monkeypatch, capsys):
    # ordinal 100 -> 8: the label loses a digit and the compiler pads its comment differently; the unit that now
    # holds _Z1bv is the second of two concatenated ones
    old = kernel("_Z1av", 3) + kernel("_Z1bv", 100, pad="  ")
    new = kernel("_Z1bv", 8, pad="    ") + kernel("_Z1av", 0, pad="\t")
    status, out, rep = run(tmp_path, monkeypatch, capsys, old, new)
    assert status == 0, out
    assert all(rep[k]["equal"] for k in ("_Z1av", "_Z1bv")) and len(rep) == 2
    assert rep["_Z1bv"]["old"] == rep["_Z1bv"]["new"] and rep["_Z1bv"]["new"]["vgprs"] == 8
    assert rep["_Z1bv"]["new"]["instructions"] == 4


def test_changed_instruction_differs(tmp_path, monkeypatch, capsys):
    old = kernel("_Z1av", 0) + kernel("_Z1bv", 1)
    new = kernel("_Z1av", 0) + kernel("_Z1bv", 1, body=("v_add_u32_e32 v1, v0, v2",))
    status, out, rep = run(tmp_path, monkeypatch, capsys, old, new)
    assert status == 1
    assert "DIFFERS _Z1bv" in out and "equal   _Z1av" in out
    assert rep["_Z1av"]["equal"] and not rep["_Z1bv"]["equal"]


@pytest.mark.parametrize("side", ["old", "new"])
def test_kernel_on_one_side_only(tmp_path, monkeypatch, capsys, side):
    both, one = kernel("_Z1av", 0) + kernel("_Z1bv", 1), kernel("_Z1av", 0)
    old, new = (both, one) if side == "old" else (one, both)
    status, out, rep = run(tmp_path, monkeypatch, capsys, old, new)
    assert status == 1
    assert rep["_Z1bv"]["missing_in"] == ("new" if side == "old" else "old")
    assert rep["_Z1av"]["equal"]


@pytest.mark.parametrize("side", ["old", "new"])
def test_duplicate_kernel_is_refused(tmp_path, monkeypatch, capsys, side):
    # the same kernel in two concatenated units: counted once, it would hide a double instantiation
    once, twice = kernel("_Z1av", 0) + kernel("_Z1bv", 1), kernel("_Z1av", 0) + kernel("_Z1bv", 1) + kernel("_Z1bv", 0)
    old, new = (twice, once) if side == "old" else (once, twice)
    status, out, _ = run(tmp_path, monkeypatch, capsys, old, new)
    assert status not in (0, None)
    assert "_Z1bv" in out and "twice" in out


def test_rename_pairs_old_with_new(tmp_path, monkeypatch, capsys):
    old = kernel("_Z1kILi0ELb1EEvv", 0, body=("s_getpc_b64 s[0:1]", "s_add_u32 s0, s0, _Z1kILi0ELb1EEvv@rel32@lo+4"))
    new = kernel("_Z1kILb1EEvv", 0, body=("s_getpc_b64 s[0:1]", "s_add_u32 s0, s0, _Z1kILb1EEvv@rel32@lo+4"))
    status, out, rep = run(tmp_path, monkeypatch, capsys, old, new)
    assert status == 1 and len(rep) == 2  # without --rename: one removed, one added
    status, out, rep = run(tmp_path, monkeypatch, capsys, old, new, "--rename", "_Z1kILi0ELb1EEvv=_Z1kILb1EEvv")
    assert status == 0, out
    assert list(rep) == ["_Z1kILb1EEvv"] and rep["_Z1kILb1EEvv"]["equal"]
    assert rep["_Z1kILb1EEvv"]["renamed_from"] == "_Z1kILi0ELb1EEvv"
    # a renamed kernel whose instructions changed still differs
    new2 = kernel("_Z1kILb1EEvv", 0, body=("s_getpc_b64 s[0:1]", "s_add_u32 s0, s0, 8"))
    status, out, rep = run(tmp_path, monkeypatch, capsys, old, new2, "--rename", "_Z1kILi0ELb1EEvv=_Z1kILb1EEvv")
    assert status == 1 and not rep["_Z1kILb1EEvv"]["equal"]
