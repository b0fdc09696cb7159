#!/usr/bin/env python3
"""Writes machisplin_amd/csrc/svr_rt_loop5.inc and svr_rt_loop5q.inc: the support-vector loop of svr_rt_tile over ONE staged
chunk (at most 128 support vectors of one sign) at P = 5, R = 3, as ONE inline-asm string for gfx950.  svr_rt_loop5.inc is
the loop of a wave that folded its cells' q into the per-wave term, svr_rt_loop5q.inc the loop that keeps q + ap per pair.

The arithmetic is the compiler's loop, instruction for instruction (the same fma's with the same operands, the clamp, the
16-bit shift, the shift-add that drops the exponent onto the table entry, the same order of additions): per (cell, support
vector) pair 12 vector instructions folded, 13 unfolded; per trip of 4 support vectors x 3 cells 145 / 157 with the one
cursor add.  What differs is when instructions issue:

  * a pair is split in two halves: A (the argument chain, t, kd, the table offset, r, and the table's ds_read_b64) and
    B (the wait, the shift-add, the polynomial and the accumulating fma).  The stream is A(p + 2), B(p) on three register
    sets: two table reads are in flight, and two argument chains have issued, before pair p's entry is consumed, and B
    waits with a COUNTED lgkmcnt(N), N = the LDS reads issued behind its own (LDS returns are in order);
  * the record of support vector k + 1 (b_0 .. b_3, one s_load_dwordx8 into the other half of a 2 x 8 SGPR buffer) and its
    per-wave term ap (one broadcast ds_read_b64 into the other of two registers) are requested at the head of support
    vector k.  A scalar load returns out of order with the LDS reads and shares lgkmcnt with them, so only lgkmcnt(0) is
    known to have retired it: that ONE drain per support vector sits in the A half of support vector k's last pair,
    directly ahead of its table read, where the reads it drains with it are 12 and 24 vector instructions old.  While the
    scalar load is in flight the counted waits are stricter than needed by one read (never laxer: the count is of
    everything outstanding), which leaves one table read in flight instead of two.

A chunk of n support vectors runs nt = (n - 1) >> 2 pipelined trips and then rem = n - 4 nt = 1 .. 4 support vectors in a
simple form (the support vector's own record and ap, drained; its three pairs overlapped among themselves): so the
read-ahead of the last pipelined trip always finds a support vector of the chunk -- no scalar load leaves the model's
records, no LDS read the wave's 128 doubles.

Registers.  Clobbered: s[84:91] / s[92:99] the two records, s100 the byte offset of the next record to request;
v[102:103] / v[104:105] the two ap, v[106:111] / v[112:117] / v[118:123] the three pair sets (arg, then the table entry; t,
whose high word becomes the table offset, then the polynomial; kd, then r), v[124:125] RT_EXP_MAGIC and v[126:127]
RT_EXP_C1 (set at the head of the block from the immediates %[mglo] .. %[c1hi]: held by the compiler they live, and
spill, across the whole kernel).  Operands: %[a0..a2] the sums (+v), %[x00..x23] the cells' scaled predictors x[c][j],
%[q0..q2] (unfolded only), %[ca] the LDS byte address of the wave's aw (+v), %[nt] pipelined trips (+s), %[rem] (s),
%[sp] the chunk's first record (s pair), %[st] bytes per record (s), %[nk] NK, %[nm] -RT_EXP_MAGIC, %[c2] C2 (s pairs).
The exponential's table sits at LDS address 0 (the kernel checks that when it is compiled)."""
import os

SB = (84, 92)
OFF = "s100"
AP = (102, 104)
PSETS = (106, 112, 118)
MG, C1 = "v[124:125]", "v[126:127]"


def rng(lo, n=2, f="v"):
    return f"{f}[{lo}:{lo + n - 1}]"


class Stream:
    """the instruction list, and the LDS reads in issue order: what a counted wait counts"""

    def __init__(self, fold):
        self.fold, self.o, self.lds = fold, [], []

    def request(self, buf, aw_off):
        """record and ap of the next support vector into buffer `buf`"""
        self.o += [f"s_load_dwordx8 {rng(SB[buf], 8, 's')}, %[sp], {OFF}", f"s_add_u32 {OFF}, {OFF}, %[st]",
                   f"ds_read_b64 {rng(AP[buf])}, %[ca] offset:{aw_off}"]
        self.lds.append("ap")

    def drain(self):
        self.o.append("s_waitcnt lgkmcnt(0)")

    def half_a(self, tag, c, buf, ps, drain=False):
        p = PSETS[ps]
        b = [rng(SB[buf] + 2 * j, 2, "s") for j in range(4)]
        ap, arg, t, k = rng(AP[buf]), rng(p), rng(p + 2), rng(p + 4)
        x = [f"%[x{c}{j}]" for j in range(4)]
        if self.fold:
            self.o.append(f"v_fma_f64 {arg}, {b[0]}, {x[0]}, {ap}")
        else:
            self.o += [f"v_add_f64 {arg}, %[q{c}], {ap}", f"v_fmac_f64_e32 {arg}, {b[0]}, {x[0]}"]
        self.o += [f"v_fmac_f64_e32 {arg}, {b[1]}, {x[1]}",
                   f"v_fmac_f64_e32 {arg}, {b[2]}, {x[2]}",
                   f"v_fma_f64 {arg}, {b[3]}, {x[3]}, {arg} clamp",
                   f"v_fma_f64 {t}, %[nk], {arg}, {MG}",
                   f"v_add_f64 {k}, {t}, %[nm]",
                   f"v_lshlrev_b16 v{p + 3}, 3, v{p + 2}",
                   f"v_fma_f64 {k}, {arg}, %[nk], -{k}"]
        if drain:
            self.drain()
        self.o.append(f"ds_read_b64 {arg}, v{p + 3}")              # arg is dead: the table entry takes its place
        self.lds.append(tag)

    def half_b(self, tag, c, ps):
        p = PSETS[ps]
        m, t, k = rng(p), rng(p + 2), rng(p + 4)
        behind = len(self.lds) - 1 - max(i for i, e in enumerate(self.lds) if e == tag)
        self.o += [f"s_waitcnt lgkmcnt({behind})",
                   f"v_lshl_add_u32 v{p + 1}, v{p + 2}, 8, v{p + 1}",      # the last use of t's low word: the polynomial takes t's place
                   f"v_fma_f64 {t}, %[c2], {k}, {C1}",
                   f"v_fma_f64 {t}, {t}, {k}, 1.0",
                   f"v_fmac_f64_e32 %[a{c}], {m}, {t}"]


def trip(s, first_b=0):
    """12 slots: A(p), B(p - 2); the slots before `first_b` come without their B (the prologue)"""
    for p in range(12):
        k, c = divmod(p, 3)
        if c == 0:
            s.request((k + 1) & 1, 8 * (k + 1))
        s.half_a(p, c, k & 1, p % 3, drain=(c == 2))
        if p >= first_b:
            q = (p - 2) % 12
            s.half_b(q, q % 3, q % 3)


def loop(fold):
    warm = Stream(fold)
    trip(warm, first_b=2)                              # the reads a trip finds behind it: those of the trip before
    s = Stream(fold)
    s.lds = list(warm.lds)
    s.o = ["v_mov_b32_e32 v124, %[mglo]", "v_mov_b32_e32 v125, %[mghi]", "v_mov_b32_e32 v126, %[c1lo]", "v_mov_b32_e32 v127, %[c1hi]",
           f"s_mov_b32 {OFF}, 0", "s_cmp_eq_u32 %[nt], 0", "s_cbranch_scc1 3f"]
    # prologue: SV 0's record and ap, drained; the first two slots of a trip without their B halves; into the trip at slot 2
    s.o += [f"s_load_dwordx8 {rng(SB[0], 8, 's')}, %[sp], {OFF}", f"s_add_u32 {OFF}, {OFF}, %[st]", f"ds_read_b64 {rng(AP[0])}, %[ca]"]
    s.drain()
    pro = Stream(fold)
    pro.request(1, 8)
    pro.half_a(0, 0, 0, 0)
    pro.half_a(1, 1, 0, 1)
    s.o += pro.o + ["s_branch 2f", "1:"]
    n0 = len(s.o)
    trip(s)
    at = next(i for i in range(n0, len(s.o)) if s.o[i].startswith("v_fma_f64 " + rng(PSETS[2])) or s.o[i].startswith("v_add_f64 " + rng(PSETS[2])))
    s.o.insert(at, "2:")                               # slot 2: the first instruction of pair 2's A half
    s.o += ["v_add_u32_e32 %[ca], 32, %[ca]", "s_sub_u32 %[nt], %[nt], 1", "s_cmp_lg_u32 %[nt], 0", "s_cbranch_scc1 1b"]
    s.half_b(10, 1, 1)
    s.half_b(11, 2, 2)                                 # lgkmcnt(0): the read-ahead (the first of the rest) is drained with it
    s.o += [f"s_sub_u32 {OFF}, {OFF}, %[st]", "3:"]    # the rest requests its own first record again
    for j in range(4):                                 # the rest, 1 .. 4 support vectors, each on its own
        s.request(0, 8 * j)
        s.drain()
        s.half_a("t0", 0, 0, 0)
        s.half_a("t1", 1, 0, 1)
        s.half_b("t0", 0, 0)
        s.half_a("t2", 2, 0, 2)
        s.half_b("t1", 1, 1)
        s.half_b("t2", 2, 2)
        if j < 3:
            s.o += [f"s_cmp_eq_u32 %[rem], {j + 1}", "s_cbranch_scc1 9f"]
    s.o += ["9:"]
    return s.o


def vector_instructions(lines, first, last):
    body = lines[lines.index(first) + 1:lines.index(last)]
    return sum(1 for ln in body if ln.startswith("v_"))


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, fold in (("svr_rt_loop5.inc", True), ("svr_rt_loop5q.inc", False)):
        lines = loop(fold)
        with open(os.path.join(root, "machisplin_amd", "csrc", name), "w") as f:
            f.write("// generated by tools/gen_svr_rt_asm.py -- do not edit\n")
            for ln in lines:
                f.write('"' + ln + '\\n\\t"\n')
        print(name, len(lines), "lines,", vector_instructions(lines, "1:", "s_sub_u32 %[nt], %[nt], 1"), "vector instructions per trip")
