"""Static instruction census of one kernel in an assembly listing, split at the clock reads (the STAMP
sections of mpc_ipm3.hip, in listing order; the unrolled Cholesky repeats its two rows per tile).  No GPU.

Usage: python tools/v3_census.py LISTING.s MANGLED_KERNEL_NAME [OPCODE ...]
  LISTING.s  e.g. `make check-hazards` leaves colaborativempc-_amd/lib/obj/mpc_ipm3_s6.s; the bench's kernel is
             _ZN4cmpc15mpc_ipm3_kernelILi4ELi4ELi2ELi2ELb0ELb1ELb0ELb0ELb1EEEvNS_8MpcConstENS_7MpcPtrsE
  OPCODE     further opcodes to count over the whole kernel (the three the DESIGN table follows are always
             printed)"""
import collections
import re
import sys

COLS = ["total", "fp64", "mfma", "acc_rd", "acc_wr", "rdlane", "wrlane", "cndmask", "valu", "lds"]
FOLLOW = ["v_accvgpr_read_b32", "ds_read2_b64", "v_cmp_eq_u32_e64"]


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_accvgpr_read"):
        return "acc_rd"
    if op.startswith("v_accvgpr_"):
        return "acc_wr"
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
        return "rdlane"
    if op.startswith("v_writelane"):
        return "wrlane"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith("v_") and "_f64" in op and not op.startswith("v_cmp") and not op.startswith("v_cvt"):
        return "fp64"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    return None


def census(path, kernel):
    secs, ops, meta, inside = [[0, collections.Counter()]], collections.Counter(), {}, False
    for no, line in enumerate(open(path), 1):
        if not inside:
            inside = line.startswith(kernel + ":")
            secs[0][0] = no
            continue
        m = re.match(r"\s+([a-z][a-z0-9_]+)(\s|$)", line)
        if not m:
            continue
        op = m.group(1)
        if op == "s_endpgm":
            break
        if op == "s_memtime":
            secs.append([no, collections.Counter()])
        ops[op] += 1
        secs[-1][1]["total"] += 1
        if classify(op):
            secs[-1][1][classify(op)] += 1
    want = re.compile(r"\s+\.(vgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)")
    blocks = open(path).read().split("  - .agpr_count:")
    for blk in blocks[1:]:
        if re.search(r"\.name:\s+" + re.escape(kernel) + r"\s", blk):
            meta = {k: int(v) for k, v in want.findall("  - .agpr_count:" + blk)}
    return secs, ops, meta


if __name__ == "__main__":
    secs, ops, meta = census(sys.argv[1], sys.argv[2])
    if not ops:
        sys.exit(f"kernel {sys.argv[2]} not found in {sys.argv[1]}")
    print(f"{sum(ops.values())} instructions; " + ", ".join(f"{k} {v}" for k, v in sorted(meta.items())))
    print("section  line  " + " ".join(f"{c:>7s}" for c in COLS))
    for i, (no, cnt) in enumerate(secs):
        print(f"{i:7d} {no:6d} " + " ".join(f"{cnt[c]:7d}" for c in COLS))
    tot = collections.Counter()
    for _, cnt in secs:
        tot.update(cnt)
    print("    all        " + " ".join(f"{tot[c]:7d}" for c in COLS))
    print("whole kernel: " + ", ".join(f"{o} {ops[o]}" for o in FOLLOW + sys.argv[3:]))
    f64 = {o: n for o, n in ops.items() if classify(o) == "fp64"}
    print("fp64: " + ", ".join(f"{o} {n}" for o, n in sorted(f64.items(), key=lambda t: -t[1])))
