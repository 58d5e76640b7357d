#!/usr/bin/env python3
"""Check the wait states around hand-written DPP instructions in a gfx950 assembly listing.

The fused broadcast-fma of csrc/wave_ops.h is inline asm, which the compiler's hazard recognizer
does not look into (and whose VGPR result it does not treat as a VALU write).  This script reads the
output of `hipcc -S --cuda-device-only` and checks, for every DPP instruction, compiler-emitted or
not:

  R1  no VALU write of the DPP source (src0) in the 2 wait states before it;
  R2  no VALU write of EXEC (v_cmpx) in the 5 wait states before it;
and for every instruction inside an inline-asm block:
  R3  no MFMA write of a register it reads in the 20 wait states before it (the compiler pads
      its own reads of an MFMA result, not the asm's);
  R4  no transcendental result (v_rcp/v_rsq/v_sqrt/...) read in the wait state directly behind it.

An instruction counts one wait state, s_nop N counts N + 1.  Blocks are followed in layout order
and, from every branch, into the first wait states of its target.  Exit status 1 on a violation.

    hipcc ... -S --cuda-device-only -o out.s file.hip && tools/check_dpp_hazards.py out.s
"""
import re
import sys

WINDOW = 20
TRANS = re.compile(r"^v_(rcp|rsq|sqrt|exp|log|sin|cos)(_|$)")
REG = re.compile(r"\b([va])(?:(\d+)|\[(\d+):(\d+)\])")


def regs(text):
    out = set()
    for m in REG.finditer(text):
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        out.update((m.group(1), i) for i in range(lo, hi + 1))
    return out


class Inst:
    __slots__ = ("line", "mn", "ops", "asm", "text")

    def __init__(self, line, text, asm):
        self.line, self.text, self.asm = line, text, asm
        parts = text.split(None, 1)
        self.mn = parts[0]
        self.ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []

    @property
    def wait_states(self):
        return int(self.ops[0], 0) + 1 if self.mn == "s_nop" else 1

    @property
    def is_valu(self):
        return self.mn.startswith("v_")

    @property
    def is_mfma(self):
        return self.mn.startswith(("v_mfma", "v_smfmac"))

    @property
    def is_dpp(self):
        return self.is_valu and ("_dpp" in self.mn or re.search(r"\b(row_|quad_perm|wave_)", self.text) is not None)

    def writes(self):
        if not self.is_valu or not self.ops:
            return set()
        w = regs(self.ops[0])
        if "swap" in self.mn and len(self.ops) > 1:
            w |= regs(self.ops[1])
        return w

    def reads(self):
        if not self.is_valu:
            return set()
        r = set()
        for o in self.ops[1:]:
            r |= regs(o.split()[0] if o else o)
        if self.mn.startswith(("v_fmac", "v_mac", "v_mfma", "v_smfmac")) and self.ops:
            r |= regs(self.ops[0])
        return r

    def dpp_src(self):
        return regs(self.ops[1].split()[0]) if len(self.ops) > 1 else set()


def parse(path):
    """-> {function: [Inst | ('label', name)]}"""
    funcs, cur, asm = {}, None, False
    for n, raw in enumerate(open(path), 1):
        line = raw.split(";", 1)[0] if "#ASM" not in raw else raw
        s = line.strip()
        if "#ASMSTART" in raw:
            asm = True
            continue
        if "#ASMEND" in raw:
            asm = False
            continue
        if not s:
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            name = m.group(1)
            if not name.startswith("."):
                cur = funcs.setdefault(name, [])
            elif cur is not None:
                cur.append(("label", name))
            continue
        if s.startswith(".") or cur is None:
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".section"):
                cur = None if s.startswith(".section") and ".text" not in s else cur
            continue
        cur.append(Inst(n, s, asm))
    return funcs


def check(items, name, report):
    labels = {it[1]: i for i, it in enumerate(items) if isinstance(it, tuple)}

    def scan(start, valu, mfma, trans, execw, limit):
        """valu/mfma/trans: {reg: wait states since the write}; execw: since a VALU write of EXEC"""
        used = 0
        for it in items[start:]:
            if limit is not None and used >= limit:
                return
            if isinstance(it, tuple):
                continue
            if it.is_dpp:
                bad = [r for r in it.dpp_src() if valu.get(r, 99) < 2]
                if bad:
                    report(name, it, f"R1: DPP source written {min(valu[r] for r in bad)} wait state(s) before")
                if execw < 5:
                    report(name, it, f"R2: EXEC written by a VALU instruction {execw} wait state(s) before")
            if it.asm and it.is_valu:
                bad = [r for r in it.reads() if mfma.get(r, 99) < WINDOW]
                if bad:
                    report(name, it, f"R3: reads an MFMA result {min(mfma[r] for r in bad)} wait state(s) old")
                bad = [r for r in it.reads() if trans.get(r, 99) < 1]
                if bad:
                    report(name, it, "R4: reads a transcendental result directly behind it")
            ws = it.wait_states
            for d in (valu, mfma, trans):
                for r in list(d):
                    d[r] += ws
                    if d[r] > WINDOW:
                        del d[r]
            execw += ws
            used += ws
            # a write lands after this instruction's own wait state: the next instruction sees age 0
            if it.is_mfma:
                mfma.update((r, 0) for r in it.writes())
            elif it.is_valu:
                w = it.writes()
                valu.update((r, 0) for r in w)
                for r in w:
                    mfma.pop(r, None)
                if TRANS.match(it.mn):
                    trans.update((r, 0) for r in w)
                if it.mn.startswith("v_cmpx"):
                    execw = 0
            if limit is None and it.mn.startswith(("s_cbranch", "s_branch")) and it.ops and it.ops[0] in labels:
                scan(labels[it.ops[0]], dict(valu), dict(mfma), dict(trans), execw, WINDOW)

    scan(0, {}, {}, {}, 99, None)


def main(paths):
    found, stats = [], {"functions": 0, "dpp": 0, "asm_dpp": 0}

    def report(fn, it, what):
        found.append(f"{fn}: line {it.line}: {it.text}\n    {what}")

    for p in paths:
        for name, items in parse(p).items():
            insts = [it for it in items if not isinstance(it, tuple)]
            if not insts:
                continue
            stats["functions"] += 1
            stats["dpp"] += sum(it.is_dpp for it in insts)
            stats["asm_dpp"] += sum(it.is_dpp and it.asm for it in insts)
            check(items, name, report)
    print(f"{stats['functions']} functions, {stats['dpp']} DPP instructions ({stats['asm_dpp']} in inline asm), "
          f"{len(found)} violation(s)")
    for f in sorted(set(found)):
        print(f)
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
