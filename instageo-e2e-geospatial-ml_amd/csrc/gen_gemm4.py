#!/usr/bin/env python3
"""Generator of the hand-scheduled K-loops of the 4-wave, one-wave-per-SIMD kernels: gemm4.hip (forward linears and data gradients,
pritvhi.py:446-456; plain and paired-split forms), gemm4w_kernel in gemm8w.hip (grouped weight gradients: the "w" / "wp" forms) and
conv4_kernel in conv8.hip (the decode head's 3 x 3 convolutions, model.py:349-390: the "c" / "cp" forms).

hipcc cannot hold 256 accumulators + 128 fragment registers of a 128 x 128-per-wave tile without spilling (rounds 2 and 5), so the K-loop of a
tile is ONE inline-asm block with hand-assigned registers; this script writes it (`gemm4_gen.inc`: string macros for the prologue and the tile
loop + the accumulator read-out helpers of the C++ epilogues).  Run by the Makefile; the output is not committed.

Layout of this file.  Everything the six forms share exists once, in the first half:
  * `weave`: a run of MFMAs with fragment reads, (M0 write, LDS-DMA) pairs and a tail hung behind chosen MFMAs -- the M0 hazard rule lives here;
  * `plain_body` / `paired_body`: the two shapes of an iteration (two halves on two fragment sets / three products on five quarter sets);
  * `gen_loop`: entry, first pair, loop over the middle pairs, last pair on the next tile's operands, exit -- with the ring rotation;
  * `gen_prologue`: K-tiles 0 and 1 of a workgroup's first tile;  `clobbers`;  the `abl_*` timing ablations (in `weave` and `sync`).
The second half is the six forms: three operand families (`Lin`: rows through a pointer; `Wg`: reduce-strided rows through a descriptor,
transposed reads; `Cv`: gathered rows), each instantiated twice (plain / paired) from a register map.  A family says how its operands are
addressed, read and fetched; it does not schedule anything.

Structure of a tile (256 x 256 x K, BK = 64, 4 waves, wave (wr, wc) owns C[wr 128 ..][wc 128 ..] as 8 x 8 MFMA 16x16x32 accumulators = a0..a255):
  LDS (160 KiB): a ring of THREE A slots (256 rows x 128 B = 32 KiB each, at 0 / 32 / 64 KiB) and TWO B stages (96 / 128 KiB); rows swizzled
  (16-byte chunk ^= row & 7).  The slot of A K-tile g (counted over the workgroup's whole tile sequence) is g mod 3: three scalar registers
  hold the slot offsets of K-tiles kt, kt + 1, kt + 2 and rotate once per iteration (they travel through the asm block's in/out operands from
  tile to tile); B's stage is kt & 1 (K-tiles per tile are even), so the loop body is unrolled by two.  The slot whose K-tile has just been
  consumed is free until the next tile's first iteration: it is the epilogue's staging buffer.
  Fragments: two register sets of 16 x 4 VGPRs (8 A row blocks + 8 B column blocks of ONE 32-deep k-substep); while the 64 MFMAs of a
  substep run on one set the other set is read from LDS.  Iteration kt (B stage p = kt & 1):
      H1: 64 MFMAs on set 0 (K-tile kt, substep 0)      | 16 ds_read_b128 -> set 1 (K-tile kt, substep 1)
                                                        | 8 LDS-DMA issues: A of K-tile kt + 2 -> the slot K-tile kt - 1 left
      sync: lgkmcnt(0), vmcnt(8), s_barrier             (everything but the 8 A pieces just issued has landed, for every wave;
                                                         B stage p and A slot kt are dead for every wave)
      H2: 64 MFMAs on set 1                             | 16 ds_read_b128 -> set 0 (K-tile kt + 1, substep 0)
                                                        | 8 LDS-DMA issues: B of K-tile kt + 2 -> stage p
  One barrier per K-tile.  The 16 LDS-DMA issues of a wave are spread over the WHOLE iteration (one per 8 MFMAs = 128 cycles; four waves: one
  per 32 cycles on the CU's texture-address path, which takes ~16 cycles per 1-KiB piece) -- with two 64-KiB stages all 16 had to go out in
  H2 (one per 16 cycles CU-wide: saturated) -- and A, whose rows come from HBM when no other tile of the XCD has touched them yet, has 1.5
  iterations to land instead of 0.5-1.  The DMA stream crosses the tile boundary (the last two iterations fetch K-tiles 0 and 1 of the
  workgroup's next tile, whose row clamp has its own offset registers).
  History (profiles/r06_gemm4_*.txt): the first form had two 64-KiB stages, all 16 issues in H2 and an L2 prefetch of the activation rows one
  K-tile ahead (a global_load_dword per wave and K-tile: qkv 130 -> 122 us on that form); with the ring the prefetch LOSES (d_fc1 143 -> 161 us:
  vmcnt retires in order, the HBM-latency prefetch holds back the L2-hit pieces behind it) and is gone.
"""
import sys
from collections import namedtuple

# ---- what every form shares: the scalar ring registers, the LDS map, the accumulators
S_APTR, S_BPTR, S_CNT, S_LDSW = 70, 72, 74, 75   # s[70:71], s[72:73], s74, s75
S_A0, S_A1, S_A2, S_ADST, S_T = 78, 79, 80, 81, 82          # slot offsets of A K-tiles kt, kt + 1, kt + 2; DMA destination base; scratch
S_LO = 70
B_BASE = 98304       # B stages behind the three 32-KiB A slots (0, 32 KiB, 64 KiB): stage b of a form with ni column blocks at + b ni 4 KiB
B_STAGE = 32768      # ... of the forms with 8 column blocks
ROWS8 = [i * 1024 for i in range(8)]   # LDS-DMA destinations of a wave's 8 pieces of 8 rows x 128 B
ADST_NEXT = f"s_add_u32 s{S_ADST}, s{S_LDSW}, s{S_A2}"   # this iteration's A pieces go to the slot K-tile kt - 1 left

# schedule keys (tools/gemm4_sweep.sh, tools/gemm4w_sweep.sh) and the four timing ablations (garbage results; profiles/README.md):
# abl_rd = no fragment reads, abl_dma = no LDS-DMA issues, abl_vmw = no vmcnt wait, abl_bar = no barrier -- honoured by every form
DEFAULTS = {"rd_every": 3, "rd_at": 0, "dm_every": 8, "dm_at": 3,
            "w_rd_at": 0, "w_rd_num": 2, "w_rd_den": 1, "w_dm_at": 3, "w_dm_every": 8, "wp_rd_num": 1, "wp_rd_den": 1,
            "abl_rd": 0, "abl_dma": 0, "abl_vmw": 0, "abl_bar": 0}


class Stream:
    def __init__(self):
        self.lines = []

    def e(self, *s):
        self.lines.extend(s)

    def text(self):
        return "\n".join(f'    "{l}\\n\\t"' for l in self.lines)


def vq(base, i):
    """block i of the fragment (quarter) set at `base`: 4 VGPRs"""
    return f"v[{base + 4 * i}:{base + 4 * i + 3}]"


def acc(mi, ni):
    b = (mi * 8 + ni) * 4
    return f"a[{b}:{b + 3}]"


def mfmas(bbase, abase, ni):
    """operands (acc, B fragment, A fragment) of acc += B[bbase] x A[abase], ni-major over 8 x ni accumulator blocks"""
    return [(acc(mi, b), vq(bbase, b), vq(abase, mi)) for b in range(ni) for mi in range(8)]


def lds_dma(dst, offs, issue, pre=lambda i: []):
    """the pieces of one operand K-tile as (pre, M0 write, issue): piece i lands at LDS address s<dst> + offs[i]"""
    return [(pre(i), f"s_add_u32 m0, s{dst}, {o}", issue(i)) for i, o in enumerate(offs)]


def by_pointer(voff, sptr):
    return lambda i: f"global_load_lds_dwordx4 v{voff + i}, s[{sptr}:{sptr + 1}]"


def by_descriptor(voff, rs):
    return lambda i: f"buffer_load_dwordx4 v{voff + i}, s[{rs}:{rs + 3}], 0 offen lds"


# ---- the three position rules: (k-th of cnt items, n MFMAs) -> index of the MFMA the item goes behind
def stride(at, num, den=1):
    """fixed stride from a start ("", p, w)"""
    return lambda k, cnt, n: at + k * num // den


def scaled(num, den):
    """evenly over the run, compressed by num / den (wp)"""
    return lambda k, cnt, n: k * n // cnt * num // den


def spread(at):
    """evenly over all but the last four MFMAs (c, cp)"""
    return lambda k, cnt, n: at + k * (n - 4) // cnt


def tail_slot(n):
    return n * 5 // 6


def weave(st, cfg, mf, first, rd, rd_pos, dm, dm_pos, tail=(), tail_at=0):
    """the MFMAs `mf` (accumulators start from 0 if `first`) with the fragment reads `rd`, the DMA pieces `dm` and `tail` hung behind them"""
    n = len(mf)
    extra = [[] for _ in range(n)]
    if cfg["abl_rd"]:
        rd = []
    if cfg["abl_dma"]:
        dm = []
    for k, r in enumerate(rd):
        extra[min(n - 1, rd_pos(k, len(rd), n))].append(r)
    for k, (pre, m0w, ld) in enumerate(dm):
        # M0 needs one instruction between its write and the LDS-DMA that reads it: the write goes LAST behind MFMA j, the issue FIRST behind
        # MFMA j + 1, so MFMA j + 1 itself is the instruction between them whatever else the two slots hold.  The piece's own address
        # arithmetic (gathered A only) goes one slot earlier still.  Positions past the run are clamped to its end: a sweep value meant for
        # one form may pile another form's pieces up there (two M0 writes in one slot), and that form's block is then good for timing only.
        j = min(n - 2, dm_pos(k, len(dm), n))
        assert j >= 1 or not pre
        extra[j - 1].extend(pre)
        extra[j].append(m0w)
        extra[j + 1].insert(0, ld)
    extra[tail_at].extend(tail)
    for j, (c, b, a) in enumerate(mf):
        st.e(f"v_mfma_f32_16x16x32_bf16 {c}, {b}, {a}, {'0' if first else c}", *extra[j])


def sync(st, cfg):
    st.e("s_waitcnt lgkmcnt(0)")
    if not cfg["abl_vmw"]:
        st.e("s_waitcnt vmcnt(8)")   # the 8 A pieces just issued may stay in flight
    if not cfg["abl_bar"]:
        st.e("s_barrier")


# ---- the two shapes of an iteration.  F is a form (second half of the file); p = B stage = K-tile parity; nxt: the DMA stream is on the next tile
Halves = namedtuple("Halves", "A B")                   # plain: fragment sets q = 0, 1 of A and of B
Quarters = namedtuple("Quarters", "AHI ALO BHI BLO")   # paired: five quarter sets, Ahi twice (alternating with the K-tile parity)
PLAIN = Halves(A=(128, 192), B=(160, 224))             # v128..v255: set q at 128 + 64 q: A blocks [0..7] x 4, then B blocks [0..7] x 4
PAIRED = Quarters(AHI=(96, 128), ALO=160, BHI=192, BLO=224)


def plain_body(F, st, p, first, nxt, cfg):
    """H1 | sync | H2 of the module docstring"""
    A, B = F.sets
    tail_at = tail_slot(8 * F.ni)
    # ---- H1: K-tile kt substep 0 | reads of substep 1 | A pieces of K-tile kt + 2 -> slot S_A2
    st.e(*F.a_addr(S_A0, 1), ADST_NEXT, *F.decode())
    weave(st, cfg, mfmas(B[0], A[0], F.ni), first, F.reads_a(A[1], 1) + F.reads_b(B[1], p, 1), F.rd_pos(cfg), F.dmas_a(nxt), F.dm_pos(cfg))
    st.e(*F.adv_a())
    sync(st, cfg)
    # ---- H2: substep 1 | reads of K-tile kt + 1 substep 0 (slot S_A1, B stage p ^ 1) | B pieces of K-tile kt + 2 -> stage p
    st.e(*F.a_addr(S_A1, 0))
    weave(st, cfg, mfmas(B[1], A[1], F.ni), False, F.reads_a(A[0], 0) + F.reads_b(B[0], p ^ 1, 0), F.rd_pos(cfg), F.dmas_b(p, nxt), F.dm_pos(cfg),
          F.tail(), tail_at)   # only H1 of a tile's first K-tile starts from 0
    st.e(*F.adv_b())


def plain_entry_reads(F):
    A, B = F.sets
    return F.a_addr(S_A0, 0) + F.reads_a(A[0], 0) + F.reads_b(B[0], 0, 0)


# PAIRED shape (the split precision mode bf16x3: value = hi + lo, products hi hi + hi lo + lo hi).  A K-tile covers 32 reduction elements; its
# 128-byte LDS row is [hi k..k+31 | lo k..k+31] (the lo lanes of an LDS-DMA piece carry the hi -> lo tensor distance in their 32-bit offset, as
# gemm8.hip's NSEG = 2), so k-substep 0 of the fragment reads is hi and substep 1 is lo, and a K-tile is THREE products of 64 MFMAs:
#     P1  acc += Bhi x Ahi      | 8 reads: Blo of this K-tile                         | 8 LDS-DMA issues: A of K-tile kt + 2
#     sync lgkmcnt(0), vmcnt(8), s_barrier
#     P2  acc += Bhi x Alo      | 8 reads: Ahi of K-tile kt + 1 -> the OTHER Ahi buffer | 4 LDS-DMA issues: B of K-tile kt + 2 (first half)
#     P3  acc += Blo x Ahi      | 16 reads: Bhi, Alo of K-tile kt + 1                   | 4 LDS-DMA issues (second half)
# Five quarter sets of 8 x 4 VGPRs (Ahi twice -- it is live from P1 to P3, so the next K-tile's copy needs a buffer of its own; the two
# alternate with the K-tile parity, which the loop is unrolled by anyway), 192 MFMAs for the 64 KiB a K-tile moves: 21 B/clk/CU at full MFMA
# rate instead of the plain form's 32 -- the paired form is NOT bound by the L2 -> LDS feed.  (The transposed reads of the wp form are two per
# fragment, so its read counts are twice these.)  P1 takes a DMA piece every 8 MFMAs, P2 / P3 every 16.
def paired_body(F, st, p, first, nxt, cfg):
    Q = F.sets
    ahi_cur, ahi_nxt = Q.AHI[p], Q.AHI[p ^ 1]
    tail_at = tail_slot(8 * F.ni)
    # a family whose read address holds no substep (Wg) points it at K-tile kt + 1 once, here: P1 reads B only
    st.e(ADST_NEXT, *([] if F.SUBSTEP_IN_ADDR else F.a_addr(S_A1, 0)), *F.decode())
    weave(st, cfg, mfmas(Q.BHI, ahi_cur, F.ni), first, F.reads_b(Q.BLO, p, 1), F.rd_pos(cfg), F.dmas_a(nxt), F.dm_pos(cfg, 8))
    st.e(*F.adv_a())
    sync(st, cfg)
    if F.SUBSTEP_IN_ADDR:
        st.e(*F.a_addr(S_A1, 0))    # A of K-tile kt + 1, hi half
    bd = F.dmas_b(p, nxt)
    h = len(bd) // 2
    weave(st, cfg, mfmas(Q.BHI, Q.ALO, F.ni), False, F.reads_a(ahi_nxt, 0), F.rd_pos(cfg), bd[:h], F.dm_pos(cfg, 16))
    if F.SUBSTEP_IN_ADDR:
        st.e(*F.a_addr(S_A1, 1))    # ... lo half (the reads above have been issued: the address is consumed at issue)
    weave(st, cfg, mfmas(Q.BLO, ahi_cur, F.ni), False, F.reads_b(Q.BHI, p ^ 1, 0) + F.reads_a(Q.ALO, 1), F.rd_pos(cfg), bd[h:], F.dm_pos(cfg, 16),
          F.tail(), tail_at)
    st.e(*F.adv_b())


def paired_entry_reads(F):
    Q = F.sets
    lo_addr = F.a_addr(S_A0, 1) if F.SUBSTEP_IN_ADDR else []
    return F.a_addr(S_A0, 0) + F.reads_a(Q.AHI[0], 0) + lo_addr + F.reads_a(Q.ALO, 1) + F.reads_b(Q.BHI, 0, 0)


def gen_loop(F, cfg, short=False):
    """one tile (Lin, Cv) or segment (Wg): the operands stand on its K-tile 2, the `next` operands on the following tile's K-tile 0.
    short: ONE K-tile pair, which is both the first and the last (Wg plain only: the walking remainder of a plan cuts such pieces)"""
    paired = isinstance(F.sets, Quarters)
    body, entry_reads = (paired_body, paired_entry_reads) if paired else (plain_body, plain_entry_reads)
    st = Stream()

    def pair(first, nxt):
        for p in (0, 1):
            body(F, st, p, first and p == 0, nxt, cfg)
            # rotate the A ring: (kt, kt + 1, kt + 2) <- (kt + 1, kt + 2, the slot kt has just left)
            st.e(f"s_mov_b32 s{S_T}, s{S_A0}", f"s_mov_b32 s{S_A0}, s{S_A1}", f"s_mov_b32 s{S_A1}, s{S_A2}", f"s_mov_b32 s{S_A2}, s{S_T}")
            st.e("s_waitcnt lgkmcnt(0)")   # the fragment set the next half's MFMAs run on has landed

    F.setup(st, True)
    if not short:
        st.e(f"s_mov_b32 s{S_CNT}, %[npair]")              # middle pairs: nk / 2 - 2
    st.e(*F.entry())
    st.e("s_waitcnt vmcnt(0)")                             # K-tiles 0, 1 (and the previous epilogue's stores)
    st.e("s_barrier")                                      # ... for every wave; every wave has left the staging slot (= S_A2)
    st.e(*entry_reads(F), "s_waitcnt lgkmcnt(0)")
    if not short:
        pair(True, False)                                  # first pair: the accumulators start from the inline constant 0
        st.e(f"s_cmp_eq_u32 s{S_CNT}, 0", "s_cbranch_scc1 L_last_%=", "L_loop_%=:")
        pair(False, False)
        st.e(f"s_sub_u32 s{S_CNT}, s{S_CNT}, 1", f"s_cmp_lg_u32 s{S_CNT}, 0", "s_cbranch_scc1 L_loop_%=", "L_last_%=:")
    st.e(*F.to_next())                                     # last pair: the DMA stream moves on to K-tiles 0, 1 of the next tile
    pair(short, True)
    # ring state for the next tile; a2 = the slot this tile's last K-tile has left = the epilogue's staging
    st.e(f"s_mov_b32 %[a0], s{S_A0}", f"s_mov_b32 %[a1], s{S_A1}", f"s_mov_b32 %[a2], s{S_A2}")
    # the last MFMAs retire before the epilogue's v_accvgpr_read (the compiler's hazard recognizer does not see into this block)
    st.e("s_nop 15", "s_nop 15")
    return st.text()


def gen_prologue(F):
    """first tile of a workgroup: A K-tiles 0 and 1 -> slots a0, a1; B K-tiles 0 and 1 -> stages 0 and 1 (the operands stand on K-tile 0).
    Nothing to hide the M0 wait state behind here: an s_nop between each M0 write and its issue"""
    st = Stream()
    F.setup(st, False)
    st.e(*F.prologue_entry())
    for k, slot in enumerate((S_A0, S_A1)):
        st.e(*F.prologue_tile(k), f"s_add_u32 s{S_ADST}, s{S_LDSW}, s{slot}")
        for pre, m0w, ld in F.dmas_a(False) + F.dmas_b(k, False):
            st.e(*pre, m0w, "s_nop 0", ld)
        st.e(*F.adv_a(), *F.adv_b())
    return st.text()


def clobbers(F):
    c = ['"memory"', '"scc"', '"m0"']
    c += [f'"a{i}"' for i in range(256)]
    c += [f'"v{i}"' for i in sorted(F.vgprs())]
    c += [f'"s{i}"' for i in range(S_LO, F.S_HI + 1)]
    return ", ".join(c)


# =====================================================================================================================================
# The forms.  A family provides: setup (offset / base registers from the block's inputs, operand pointers), a_addr (A fragment read address
# for a slot and k-substep), reads_a / reads_b, dmas_a / dmas_b, adv_a / adv_b (next K-tile), to_next (in front of the last pair), rd_pos /
# dm_pos (schedule), vgprs (for the clobber list), and the optional hooks below.  Register maps are explicit; everything a block names is in
# its clobber list: a CONTIGUOUS form declares v<TMP>..v255, the others exactly the registers they name (the compiler keeps the rest).
class Form:
    SUBSTEP_IN_ADDR = True   # the A read address is slot + substep base (Lin, Cv); Wg carries the substep in the read's offset field
    ni = 8                   # B column blocks per wave

    def __init__(self, sets, contiguous=False, **regs):
        self.sets, self.contiguous = sets, contiguous
        self.__dict__.update(regs)

    def vgprs(self):
        return range(self.TMP, 256) if self.contiguous else self.named_vgprs()

    def set_vgprs(self):
        """the fragment sets: 8 A blocks, ni B blocks of 4 registers each"""
        s = self.sets
        a, b = ((*s.AHI, s.ALO), (s.BHI, s.BLO)) if isinstance(s, Quarters) else (s.A, s.B)
        return {r for base in a for r in range(base, base + 32)} | {r for base in b for r in range(base, base + 4 * self.ni)}

    def ring_in(self):
        return [f"s_mov_b32 s{S_LDSW}, %[ldsw]", f"s_mov_b32 s{S_A0}, %[a0]", f"s_mov_b32 s{S_A1}, %[a1]", f"s_mov_b32 s{S_A2}, %[a2]"]

    # hooks only the gathered family fills
    def entry(self): return []             # extra instructions at a tile's entry
    def decode(self): return []            # at the top of an iteration
    def tail(self): return []              # behind the last product's MFMA tail_slot(n)
    def prologue_entry(self): return []
    def prologue_tile(self, k): return []


class Lin(Form):
    """rows of both operands through 64-bit pointers + per-piece VGPR offsets (forward linears, data gradients)"""
    S_HI = 82

    def fb(F, stage, s):
        return f"v{F.FB + 2 * stage + s}"

    def frag_bases(F):
        out = [f"v_mov_b32 v{F.FA}, %[fa]", f"v_xor_b32 v{F.FA + 1}, 64, %[fa]"]
        for b in (0, 1):
            out += [f"v_add_u32 {F.fb(b, 0)}, {B_BASE + b * F.ni * 4096}, %[fb]", f"v_xor_b32 {F.fb(b, 1)}, 64, {F.fb(b, 0)}"]
        return out

    def setup(F, st, with_next):
        for i in range(8):
            st.e(f"v_add_u32 v{F.TMP}, {8 * i}, %[rowv]",
                 f"v_min_u32 v{F.TMP + 1}, %[vrc], v{F.TMP}",
                 f"v_mad_u32_u24 v{F.OFFA + i}, v{F.TMP + 1}, %[lda2], {F.c16a}",
                 f"v_min_u32 v{F.TMP + 1}, %[vrn], v{F.TMP}",
                 f"v_mad_u32_u24 v{F.OFFA_N + i}, v{F.TMP + 1}, %[lda2], {F.c16a}",
                 f"v_mad_u32_u24 v{F.OFFB + i}, v{F.TMP}, %[ldb2], {F.c16b}")
        st.e(*F.frag_bases(), *F.ring_in())
        st.e(f"s_mov_b64 s[{S_APTR}:{S_APTR + 1}], %[aptr]", f"s_mov_b64 s[{S_BPTR}:{S_BPTR + 1}], %[bptr]")

    def a_addr(F, slot, s):
        return [f"v_add_u32 v{F.AC}, s{slot}, v{F.FA + s}"]

    def reads_a(F, base, s):
        """the 8 A fragment reads of a k-substep, from the slot and substep a_addr has put into AC"""
        return [f"ds_read_b128 {vq(base, i)}, v{F.AC} offset:{i * 2048}" for i in range(8)]

    def reads_b(F, base, stage, s):
        return [f"ds_read_b128 {vq(base, i)}, {F.fb(stage, s)} offset:{i * 2048}" for i in range(F.ni)]

    def dmas_a(F, nxt):
        """the wave's 64 rows of an A K-tile (8 rows x 128 B per piece) into the slot S_ADST points at"""
        return lds_dma(S_ADST, ROWS8, by_pointer(F.OFFA_N if nxt else F.OFFA, S_APTR))

    def dmas_b(F, stage, nxt):
        return lds_dma(S_LDSW, [B_BASE + stage * B_STAGE + o for o in ROWS8], by_pointer(F.OFFB, S_BPTR))

    def advance(F, ptr):
        return [f"s_add_u32 s{ptr}, s{ptr}, {F.step}", f"s_addc_u32 s{ptr + 1}, s{ptr + 1}, 0"]

    def adv_a(F):
        return F.advance(S_APTR)

    def adv_b(F):
        return F.advance(S_BPTR)

    def to_next(F):
        return [f"s_mov_b64 s[{S_APTR}:{S_APTR + 1}], %[anext]", f"s_mov_b64 s[{S_BPTR}:{S_BPTR + 1}], %[bnext]"]

    def rd_pos(F, cfg):
        return stride(cfg["rd_at"], cfg["rd_every"])

    def dm_pos(F, cfg, every=None):
        return stride(cfg["dm_at"], every or cfg["dm_every"])

    def named_vgprs(F):
        used = set(range(F.TMP, F.TMP + 2)) | set(range(F.FA, F.FA + 2)) | set(range(F.FB, F.FB + 4)) | {F.AC}
        return used | set(range(F.OFFA_N, F.OFFA_N + 8)) | set(range(F.OFFA, F.OFFA + 8)) | set(range(F.OFFB, F.OFFB + 8)) | F.set_vgprs()


# v94, v95: scratch; v96, v97: A fragment base of k-substep 0 / 1 (without the slot offset); v98..v101: B fragment bases [stage][substep];
# v102: A fragment base of the half being read (FA[s] + slot offset); v104..v111 / v112..v119: DMA offsets of A, NEXT tile's row clamp / this
# tile; v120..v127: DMA offsets of B.  Pointers advance 128 bytes per K-tile.
G4 = Lin(PLAIN, contiguous=True, TMP=94, FA=96, FB=98, AC=102, OFFA_N=104, OFFA=112, OFFB=120, c16a="%[c16]", c16b="%[c16]", step=128)
# paired: the same map 40 registers lower, under the five quarter sets at v96..v255 (the compiler keeps v63, v88..v95 among the rest);
# 64 bytes per 32-element K-tile
G4P = Lin(PAIRED, TMP=54, FA=56, FB=58, AC=62, OFFA_N=64, OFFA=72, OFFB=80, c16a="%[c16a]", c16b="%[c16b]", step=64)


# =====================================================================================================================================
# WEIGHT-GRADIENT family (gemm4w, used by gemm8w.hip for the plain 256 x 256 linears): dW[n][k] += sum_t dy[t][n] x[t][k].  The reduction runs over
# tokens, so both operands are reduce-strided: an operand tile in LDS is two halves of [64 tokens][128 columns] (256-byte rows), filled by
# LDS-DMA in full 256-byte source rows through a buffer descriptor (tokens past the segment's end read as zeros), and the MFMA fragments come
# from ds_read_b64_tr_b16 (hardware transpose; the image, its chunk-pair swizzle and the fragment addressing are gemm8w.hip's).  Wave (wr, wc)
# reads A half wr (the n side: dy) and B half wc (the k side: x).  Same ring (three A slots, two B stages), same iteration shape as the
# forward form; a fragment is two 8-byte reads, so a half-iteration carries 32 reads.  The unit of work is a SEGMENT (output tile x token
# range) of the host-built plan; the DMA stream crosses segment boundaries the way the forward form crosses tiles.
# Paired (bf16x3): a K-tile covers 32 tokens, the 64 LDS rows of a half-tile are [hi tokens 0-31 | lo tokens 0-31] (waves 0, 1 fetch from the
# hi tensors, waves 2, 3 the same token rows from the lo tensors: wave-uniform, the descriptor base selects), so k-substep 0 of the fragment
# reads is hi and substep 1 is lo.  The next segment's DMA offsets are computed in place before the last pair (no second offset set: the five
# quarter sets take v96..v255), which the map says by OFFA_N = OFFA, OFFB_N = OFFB.
WS_RA, WS_RB = 84, 88           # s[84:87], s[88:91]: buffer descriptors of the A / B stream
WS_STEPA, WS_STEPB = 92, 93     # bytes per K-tile (64 tokens x row pitch)
W_PIECES = [h * 16384 + i * 1024 for h in range(2) for i in range(4)]   # piece (h, i) of a wave: half h, token rows 4 i .. 4 i + 3


class Wg(Form):
    S_HI = 93
    SUBSTEP_IN_ADDR = False

    def offsets(F, sfx):
        """DMA offsets: piece (h, i) of this wave = token rows 16 w + 4 i + (lane >> 4), half h: row x pitch + 256 h + 16 x source chunk
        (the chunk-pair key of LDS rows 8 .. 15 of a 16-row group has bit 2 set: source chunk ^ 8, byte offset ^ 128 = TMP + 1)"""
        out = []
        for base, ld in ((F.OFFA_N if sfx else F.OFFA, f"%[lda2{sfx}]"), (F.OFFB_N if sfx else F.OFFB, f"%[ldb2{sfx}]")):
            for h in range(2):
                for i in range(4):
                    out += [f"v_add_u32 v{F.TMP}, {4 * i}, %[rowv]",
                            f"v_mad_u32_u24 v{base + h * 4 + i}, v{F.TMP}, {ld}, {f'v{F.TMP + 1}' if i >= 2 else '%[lch0]'}"]
                    if h:
                        out.append(f"v_add_u32 v{base + h * 4 + i}, 256, v{base + h * 4 + i}")
        return out

    def desc(F, sfx):
        """descriptors of the two streams: 64-bit base (stride 0), bytes, raw-buffer flags; bytes per K-tile = 64 (paired: 32) x row pitch"""
        return [f"s_mov_b64 s[{WS_RA}:{WS_RA + 1}], %[ra{sfx}]", f"s_mov_b32 s{WS_RA + 2}, %[na{sfx}]", f"s_mov_b32 s{WS_RA + 3}, 0x00020000",
                f"s_mov_b64 s[{WS_RB}:{WS_RB + 1}], %[rb{sfx}]", f"s_mov_b32 s{WS_RB + 2}, %[nb{sfx}]", f"s_mov_b32 s{WS_RB + 3}, 0x00020000",
                f"s_lshl_b32 s{WS_STEPA}, %[lda2{sfx}], {F.shift}", f"s_lshl_b32 s{WS_STEPB}, %[ldb2{sfx}], {F.shift}"]

    def setup(F, st, with_next):
        # fragment addresses: toff[i] = tbase + ((i << 5) ^ rkey5); A: + the wave's half (fah); B: + the wave's half + stage base (fbh)
        for i in range(8):
            st.e(f"v_xor_b32 v{F.TMP}, {i << 5}, %[rkey5]",
                 f"v_add_u32 v{F.TMP}, v{F.TMP}, %[tbase]",
                 f"v_add_u32 v{F.ABASE + i}, v{F.TMP}, %[fah]",
                 f"v_add_u32 v{F.TMP}, v{F.TMP}, %[fbh]",
                 f"v_add_u32 v{F.B + i}, {B_BASE}, v{F.TMP}",
                 f"v_add_u32 v{F.B + 8 + i}, {B_BASE + B_STAGE}, v{F.TMP}")
        st.e(f"v_xor_b32 v{F.TMP + 1}, 128, %[lch0]", *F.offsets(""))
        if with_next and F.OFFA_N != F.OFFA:
            st.e(*F.offsets("n"))
        st.e(*F.ring_in(), *F.desc(""))

    def a_addr(F, slot, s):
        return [f"v_add_u32 v{F.ACUR + i}, s{slot}, v{F.ABASE + i}" for i in range(8)]

    def reads_tr(F, base, addr, s):
        out = []
        for i in range(8):
            out += [f"ds_read_b64_tr_b16 v[{base + 4 * i}:{base + 4 * i + 1}], v{addr + i} offset:{s * 8192}",
                    f"ds_read_b64_tr_b16 v[{base + 4 * i + 2}:{base + 4 * i + 3}], v{addr + i} offset:{s * 8192 + 1024}"]
        return out

    def reads_a(F, base, s):
        return F.reads_tr(base, F.ACUR, s)

    def reads_b(F, base, stage, s):
        return F.reads_tr(base, F.B + 8 * stage, s)

    def dmas_a(F, nxt):
        return lds_dma(S_ADST, W_PIECES, by_descriptor(F.OFFA_N if nxt else F.OFFA, WS_RA))

    def dmas_b(F, stage, nxt):
        return lds_dma(S_LDSW, [B_BASE + stage * B_STAGE + o for o in W_PIECES], by_descriptor(F.OFFB_N if nxt else F.OFFB, WS_RB))

    def advance(F, rs, step):
        """next K-tile: base += step, num_records -= step (clamped at 0: the tokens past the segment's end read as zeros)"""
        return [f"s_add_u32 s{rs}, s{rs}, s{step}", f"s_addc_u32 s{rs + 1}, s{rs + 1}, 0",
                f"s_sub_u32 s{rs + 2}, s{rs + 2}, s{step}", f"s_cselect_b32 s{rs + 2}, 0, s{rs + 2}"]

    def adv_a(F):
        return F.advance(WS_RA, WS_STEPA)

    def adv_b(F):
        return F.advance(WS_RB, WS_STEPB)

    def to_next(F):
        """the DMA stream moves on to the next segment (ran / rbn: descriptors at its first token)"""
        in_place = [f"v_xor_b32 v{F.TMP + 1}, 128, %[lch0]", *F.offsets("n")] if F.OFFA_N == F.OFFA else []
        return F.desc("n") + in_place

    def rd_pos(F, cfg):
        if isinstance(F.sets, Quarters):
            return scaled(cfg["wp_rd_num"], cfg["wp_rd_den"])
        return stride(cfg["w_rd_at"], cfg["w_rd_num"], cfg["w_rd_den"])

    def dm_pos(F, cfg, every=None):
        return stride(cfg["w_dm_at"], every or cfg["w_dm_every"])


# v62, v63: scratch; v64..v71: A fragment address of block mi without the slot; v72..v79: with the slot of the half being read; v80..v95: B
# fragment addresses [stage][ni]; v96..v127: DMA offsets (h, i) of A / B, this and the next segment; fragment sets as the forward form's
G4W = Wg(PLAIN, contiguous=True, TMP=62, ABASE=64, ACUR=72, B=80, OFFA=96, OFFA_N=104, OFFB=112, OFFB_N=120, shift=6)
G4WP = Wg(PAIRED, contiguous=True, TMP=46, ABASE=48, ACUR=56, B=64, OFFA=80, OFFA_N=80, OFFB=88, OFFB_N=88, shift=5)


# =====================================================================================================================================
# CONVOLUTION family (conv4_kernel<NI> in conv8.hip: the decode head's 3 x 3 convolutions as implicit GEMMs on a 256 x 32 NI tile, wave (wr, wc)
# owns 128 rows x 16 NI columns = 8 x NI accumulator blocks; NI = 6 or 3).  The loop is the forward form's with two changes:
#   * A is GATHERED (conv8.hip): piece i of a wave is `buffer_load_dwordx4 v_off, s[desc], 0 offen lds` with
#         v_off = rowoff_i + delta(K chunk) + (invalid ? 2^31 : 0)
#     where (delta, mask bit) of the lane's 16-byte K chunk come from ONE table entry per lane and K-tile (read from LDS one iteration ahead),
#     invalid = bit `mask bit` of the row's INVERTED tap mask, and an offset beyond the descriptor's bound makes the hardware write zeros:
#     three vector instructions per piece (v_bfe_u32, v_lshl_add_u32, v_add_u32) woven in front of its issue.  The table index runs
#     cyclically over the nk K-tiles of a tile and wraps to the NEXT tile's table (the four sub-pixel phases of a ConvTranspose forward have
#     their own tables, K lengths and packed row pitches); the row offsets / masks and B offsets of the next tile take over for the last pair.
#   * B (packed weights [N][Kpad]) has 32 ni rows (ni = 6: the 256 x 192 tile, 3: 256 x 96): ni pieces per wave and K-tile, two stages of
#     4 ni KiB behind the A slots; the chunk table sits at 144 KiB.
# Paired (conv4_kernel<6, PAIR>: the split precision mode bf16x3 of the wide head stages): the forward paired form's K-tile (32 reduction
# elements, LDS row = [hi | lo], three products on five quarter fragment sets) with gathered A pieces: the lo lanes of a piece (source chunk
# >= 4) carry the hi -> lo tensor distance in `aloadd` / in their B offset, the table has four entries per K-tile (16 bytes: `tstride`), the
# descriptor spans both tensors.
CS_RSRC = 84          # s[84:87]: buffer descriptor of the gathered tensor
CS_TOFF, CS_LEFT, CS_NK = 88, 89, 90   # table byte offset of the next entry to read, entries left before it wraps, K-tiles per tile
CS_LDSWB = 91         # LDS-DMA destination base of this wave's B pieces (8 ni rows per wave: wave * ni KiB)


class Cv(Lin):
    """Lin's fragment reads and B pointer; A gathered through a descriptor; tile: bptr on its K-tile 2, bnext on the next tile's K-tile 0;
    ro / im = this tile's rows, ron / imn = the next tile's; toff4 = byte offset of its table; paired: nk = 32-element K-tiles, a multiple of 4"""
    S_HI = 91

    def setup(F, st, with_next):
        for i in range(F.ni):   # B rows past the tile's valid width (a ragged last column tile) re-read its last valid row: vrb = valid rows - 1
            st.e(f"v_add_u32 v{F.TMP}, {8 * i}, %[browv]",
                 f"v_min_u32 v{F.TMP + 1}, %[vrb], v{F.TMP}",
                 f"v_mad_u32_u24 v{F.OFFB + i}, v{F.TMP + 1}, %[ldb2], {F.c16b}")
            if with_next:
                st.e(f"v_min_u32 v{F.TMP + 1}, %[vrbn], v{F.TMP}",
                     f"v_mad_u32_u24 v{F.OFFB_N + i}, v{F.TMP + 1}, %[ldb2n], {F.c16b}")
        st.e(*F.frag_bases(), *F.ring_in())
        st.e(f"s_mov_b64 s[{CS_RSRC}:{CS_RSRC + 1}], %[abase]", f"s_mov_b32 s{CS_RSRC + 2}, %[abytes]", f"s_mov_b32 s{CS_RSRC + 3}, 0x00020000",
             f"s_mov_b32 s{CS_NK}, %[nk]", f"s_mov_b32 s{CS_LDSWB}, %[ldswb]", f"s_mov_b64 s[{S_BPTR}:{S_BPTR + 1}], %[bptr]")

    def dmas_a(F, nxt):
        """8 x (3 VALU, M0 write, issue): TMP = delta bytes, TMP + 1 = mask bit of this K-tile's entry (`decode`, at the top of the iteration)"""
        sfx = "n" if nxt else ""
        return lds_dma(S_ADST, ROWS8, by_descriptor(F.O, CS_RSRC), lambda i: [
            f"v_bfe_u32 v{F.O + i}, %[im{sfx}{i}], v{F.TMP + 1}, 1",
            f"v_lshl_add_u32 v{F.O + i}, v{F.O + i}, 31, v{F.TMP}",
            f"v_add_u32 v{F.O + i}, v{F.O + i}, %[ro{sfx}{i}]"])

    def dmas_b(F, stage, nxt):
        return lds_dma(CS_LDSWB, [B_BASE + stage * F.ni * 4096 + o for o in ROWS8[:F.ni]], by_pointer(F.OFFB_N if nxt else F.OFFB, S_BPTR))

    def adv_a(F):
        return []

    def to_next(F):
        return [f"s_mov_b64 s[{S_BPTR}:{S_BPTR + 1}], %[bnext]"]

    def decode(F):
        out = [f"v_ashrrev_i32 v{F.TMP}, 8, v{F.E}",           # displacement in 16-byte units (signed)
               f"v_lshlrev_b32 v{F.TMP}, 4, v{F.TMP}"]
        if isinstance(F.sets, Quarters):
            out.append(f"v_add_u32 v{F.TMP}, v{F.TMP}, %[aloadd]")   # lanes that fetch lo: + the distance of the lo tensor
        return out + [f"v_and_b32 v{F.TMP + 1}, 31, v{F.E}"]    # bit of the row's inverted tap mask (31: padding chunk, always invalid)

    def tail(F):
        """advance the cyclic table offset and read the entry of the K-tile whose A pieces the NEXT iteration issues"""
        return [f"s_add_u32 s{CS_TOFF}, s{CS_TOFF}, {F.tstride}", f"s_sub_u32 s{CS_LEFT}, s{CS_LEFT}, 1", f"s_cmp_eq_u32 s{CS_LEFT}, 0",
                f"s_cselect_b32 s{CS_TOFF}, %[toffn4], s{CS_TOFF}", f"s_cselect_b32 s{CS_LEFT}, s{CS_NK}, s{CS_LEFT}",
                f"v_add_u32 v{F.TA}, s{CS_TOFF}, %[vtl]", f"ds_read_b32 v{F.E}, v{F.TA}"]

    def entry(F):
        return [f"s_add_u32 s{CS_TOFF}, %[toff4], {2 * F.tstride}",        # the first iteration issues K-tile 2 of this tile's table
                f"s_sub_u32 s{CS_LEFT}, s{CS_NK}, 2", f"v_add_u32 v{F.TA}, s{CS_TOFF}, %[vtl]", f"ds_read_b32 v{F.E}, v{F.TA}"]

    def prologue_entry(F):
        return [f"v_add_u32 v{F.TA}, %[toff4], %[vtl]"]

    def prologue_tile(F, k):
        """table entries 0 and 1 of the tile's phase"""
        return [f"ds_read_b32 v{F.E}, v{F.TA} offset:{F.tstride * k}", "s_waitcnt lgkmcnt(0)", *F.decode()]

    def rd_pos(F, cfg):
        return spread(0)

    def dm_pos(F, cfg, every=None):
        return spread(2)

    def named_vgprs(F):
        return set(range(F.TMP, F.OFFB + F.ni)) | {F.TA} | set(range(F.OFFB_N, F.OFFB_N + F.ni)) | F.set_vgprs()


def G4C(ni):
    # Lin's v94..v102; v103: table entry of the K-tile whose A pieces are issued next; v104..v111: gathered offsets of the 8 A pieces;
    # v112..v117: DMA offsets of the (up to 6) B pieces; v118: table read address; v119..v124: B offsets of the NEXT tile (another phase of a
    # ConvTranspose forward has another row pitch)
    return Cv(PLAIN, ni=ni, TMP=94, FA=96, FB=98, AC=102, E=103, O=104, OFFB=112, TA=118, OFFB_N=119, c16b="%[c16]", step=128, tstride=32)


def G4CP(ni):
    return Cv(PAIRED, ni=ni, TMP=54, FA=56, FB=58, AC=62, E=63, O=64, OFFB=72, TA=78, OFFB_N=80, c16b="%[c16b]", step=64, tstride=16)


def gen_readout():
    """C++ helpers: g4_acc_row<MI>(f32x4 (&t)[8]) reads the 8 column blocks of row block MI out of the AGPRs"""
    out = []
    for mi in range(8):
        out.append(f"__device__ __forceinline__ void g4_acc_row{mi}(f32x4 (&t)[8]) {{")
        for ni in range(8):
            b = (mi * 8 + ni) * 4
            out.append(f'    asm volatile("v_accvgpr_read_b32 %0, a{b}\\n\\tv_accvgpr_read_b32 %1, a{b + 1}\\n\\tv_accvgpr_read_b32 %2, a{b + 2}\\n\\tv_accvgpr_read_b32 %3, a{b + 3}" '
                       f': "=v"(t[{ni}][0]), "=v"(t[{ni}][1]), "=v"(t[{ni}][2]), "=v"(t[{ni}][3]));')
        out.append("}")
    out.append("__device__ __forceinline__ void g4_acc_row(int mi, f32x4 (&t)[8]) {")
    out.append("    switch (mi) {")
    for mi in range(8):
        out.append(f"        case {mi}: g4_acc_row{mi}(t); break;")
    out.append("    }")
    out.append("}")
    return "\n".join(out)


def macros(cfg):
    """(macro name, text) in file order: gemm4.hip, gemm8w.hip and conv8.hip use these names"""
    out = []
    for name, F in (("G4", G4), ("G4P", G4P), ("G4W", G4W), ("G4WP", G4WP),
                    ("G4C6", G4C(6)), ("G4C3", G4C(3)), ("G4CP6", G4CP(6)), ("G4CP3", G4CP(3))):   # conv4_kernel<NI> / <NI, true>: 256 x 192, 256 x 96
        unit = "SEG" if isinstance(F, Wg) else "TILE"
        out += [(f"{name}_ASM_PROLOGUE", gen_prologue(F)), (f"{name}_ASM_{unit}", gen_loop(F, cfg))]
        if F is G4W:
            out.append((f"{name}_ASM_SEG_SHORT", gen_loop(F, cfg, short=True)))
        out.append((f"{name}_CLOBBERS", clobbers(F)))
    return out


def main():
    cfg = dict(DEFAULTS)
    out_path = "gemm4_gen.inc"
    for a in sys.argv[1:]:
        if "=" in a:
            k, v = a.split("=", 1)
            if k not in cfg:
                sys.exit(f"gen_gemm4.py: unknown key '{k}' (known: {' '.join(cfg)})")
            cfg[k] = int(v)
        else:
            out_path = a
    with open(out_path, "w") as f:
        f.write("// GENERATED by gen_gemm4.py -- do not edit.  cfg = %r\n" % (cfg,))
        for name, text in macros(cfg):
            sep = " " if name.endswith("_CLOBBERS") else " \\\n"
            f.write(f"#define {name}{sep}" + text.replace("\n", " \\\n") + "\n\n")
        f.write(gen_readout() + "\n")


if __name__ == "__main__":
    main()
