#!/usr/bin/env python3
"""Compare the kernels of two device-assembly builds of the same HIP code.

    hipcc <HIPFLAGS of the Makefile> --cuda-device-only -S file.hip -o a.s   (old tree)
    hipcc <HIPFLAGS of the Makefile> --cuda-device-only -S file.hip -o b.s   (new tree)
    tools/kernel_isa_diff.py a.s b.s [--json out.json] [--count v_mfma ds_read ...] [--rename OLD=NEW ...]

Either side may be the `cat` of several units' assembly (a source split into, or
merged from, several translation units): kernels are matched by name, wherever
they stand.  Per kernel (symbol .. function-end label) the text is compared
after the local label numbers (.LBB<n>_) are normalised and every line's
trailing `;` comment and trailing whitespace are removed (the comments and
their padding depend on a function's ordinal in its file; comment-only lines
drop out); the resources are read from the compiler's own summary after the
function.  A kernel of one build only is listed with its resources.  Exit
status 1 when a kernel's text differs, a kernel is in one build only, or a name
occurs twice on one side (a kernel instantiated in two units).

--rename OLD=NEW compares kernel OLD of the
old build with kernel NEW of the new one (a kernel whose template parameters or
argument types were renamed): OLD is replaced by NEW in the old build's name and
text first, and the report keeps the old name under "renamed_from".
"""
import argparse
import json
import re
import sys

RES = {"vgprs": r"; NumVgprs: (\d+)", "agprs": r"; NumAgprs: (\d+)", "sgprs": r"; TotalNumSgprs: (\d+)",
       "scratch": r"; ScratchSize: (\d+)", "lds": r"; LDSByteSize: (\d+)", "code_bytes": r"; codeLenInByte = (\d+)"}


def kernels(path):
    out, name, body, tail = {}, None, [], None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None and tail is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                if name in out:
                    sys.exit(f"{path}: kernel {name} occurs twice (instantiated in two units?)")
                out[name] = {"text": body}
                tail, name = out[name], None
            else:
                text = re.sub(r"BB\d+_", "BB_", line.split(";")[0]).rstrip()
                if text:
                    body.append(text)
            continue
        if tail is not None:
            for k, pat in RES.items():
                m = re.search(pat, line)
                if m:
                    tail[k] = int(m.group(1))
            if line.startswith("; LDSByteSize"):
                tail = None
    return out


def insns(text):
    return [l.split()[0] for l in text if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--json")
    ap.add_argument("--count", nargs="*", default=["v_mfma", "ds_read", "global_load_lds", "v_med3", "v_max3"],
                    help="opcode prefixes counted for kernels whose text differs")
    ap.add_argument("--rename", nargs="*", default=[], metavar="OLD=NEW",
                    help="kernel OLD of the old build is kernel NEW of the new one")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    renamed = {}
    for pair in a.rename:
        o, n = pair.split("=", 1)
        if o in old:
            d = old.pop(o)
            d["text"] = [line.replace(o, n) for line in d["text"]]
            old[n], renamed[n] = d, o
    rep, same = {}, True
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            # a kernel of one build only (added or removed): its resources, and no verdict on the others
            side, d = ("new", new[k]) if k not in old else ("old", old[k])
            rep[k] = {"equal": False, "missing_in": "old" if k not in old else "new",
                      side: {**{r: d.get(r) for r in RES}, "instructions": len(insns(d["text"])),
                             "counts": {p: sum(o.startswith(p) for o in insns(d["text"])) for p in a.count}}}
            print(("added   " if k not in old else "removed ") + k, rep[k][side])
            same = False
            continue
        e = {"equal": old[k]["text"] == new[k]["text"]}
        for side, d in (("old", old[k]), ("new", new[k])):
            ops = insns(d["text"])
            e[side] = {r: d.get(r) for r in RES}
            e[side]["instructions"] = len(ops)
            if not e["equal"]:
                e[side]["counts"] = {p: sum(o.startswith(p) for o in ops) for p in a.count}
        if k in renamed:
            e["renamed_from"] = renamed[k]
        rep[k] = e
        same &= e["equal"]
        print(("equal   " if e["equal"] else "DIFFERS ") + k, e["old"], "->", e["new"])
    if a.json:
        json.dump({"kernels": rep}, open(a.json, "w"), indent=1)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
