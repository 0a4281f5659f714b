#!/usr/bin/env python3
"""Do two builds hold the same device code?  For every *.hip.o of this tree's build and of another built tree's, the gfx950
code object is taken out of the object file's .hip_fatbin section and disassembled; the instruction text (addresses and
encodings stripped) is hashed per unit.  Needs no GPU.

    python scripts/device_code_diff.py OTHER_TREE [--out profiles/history/device_code.json]
"""
import argparse
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROMIS_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def instructions(obj, tmp):
    """the disassembly of obj's gfx950 code object: one line per instruction or label, no address, no encoding"""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "code.o")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                           f"--input={fat}", f"--output={co}"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    lines = [re.sub(r"\s*//.*$", "", ln).strip() for ln in text.splitlines()[2:]]
    return [ln for ln in lines if ln]


def kernel_text(ins, name):
    """the lines of symbol `name` in a unit's disassembly: from its label to the next symbol's, without the padding behind
    its s_endpgm, and with the pc-relative literal behind an s_getpc_b64 (the distance to a constant table, which moves
    when another kernel joins the unit) replaced by a token"""
    out, on, getpc = [], False, -9
    for ln in ins:
        m = re.match(r"^<(\S+)>:$", ln)
        if m:
            on = m.group(1) == name
        elif on:
            if ln.startswith("s_getpc_b64"):
                getpc = len(out)
            elif len(out) - getpc <= 2 and re.match(r"^s_add_u32 (s\d+), \1, 0x[0-9a-f]+$", ln):
                ln = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ln)
            out.append(ln)
    while out and (out[-1].startswith("s_nop") or out[-1].startswith("s_code_end") or out[-1] == "..."):
        out.pop()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history", "device_code.json"))
    ap.add_argument("--kernels", nargs="*", default=[], metavar="UNIT:KERNEL",
                    help="also compare single kernels of a unit that differs, e.g. phat_table.hip.o:k_phat_table; "
                         "UNIT:KERNEL=OTHER_KERNEL where the other tree names the kernel differently (a kernel that became a "
                         "template's instantiation)")
    a = ap.parse_args()
    here = {os.path.basename(p): p for p in glob.glob(os.path.join(ROOT, "romis_amd", "_build", "*.hip.o"))}
    there = {os.path.basename(p): p for p in glob.glob(os.path.join(os.path.abspath(a.other), "romis_amd", "_build", "*.hip.o"))}
    res = {"what": "per device unit: sha256 of the gfx950 disassembly (instructions and labels, no addresses), this tree / the other",
           "units": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(set(here) | set(there)):
            rec = {}
            for label, objs in (("this", here), ("other", there)):
                if name in objs:
                    ins = instructions(objs[name], tmp)
                    rec[label] = {"sha256": hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16], "lines": len(ins)}
            rec["equal"] = "this" in rec and "other" in rec and rec["this"] == rec["other"]
            res["units"][name] = rec
        for uk in a.kernels:
            unit, _, kern = uk.partition(":")
            kern, _, other_kern = kern.partition("=")
            rec = {}
            for label, objs in (("this", here), ("other", there)):
                if unit in objs:
                    ins = kernel_text(instructions(objs[unit], tmp), other_kern if label == "other" and other_kern else kern)
                    rec[label] = {"sha256": hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16], "lines": len(ins)}
            rec["equal"] = "this" in rec and "other" in rec and rec["this"] == rec["other"] and rec["this"]["lines"] > 0
            res.setdefault("kernels", {})[uk] = rec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    for name, rec in res["units"].items():
        print(name, "equal" if rec["equal"] else ("only here" if "other" not in rec else "only there" if "this" not in rec else "DIFFERENT"),
              rec.get("this", {}).get("lines"))
    for uk, rec in res.get("kernels", {}).items():
        print(uk, "equal" if rec["equal"] else "DIFFERENT", rec.get("this", {}).get("lines"), rec.get("other", {}).get("lines"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
