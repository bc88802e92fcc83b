"""lstm_head_train_step (csrc/bindings.cpp), the step bench.py times, against
the fp64 reference of tests/_head_step_ref.py: every element of the flat
gradient within its budget, the statistics [mean loss, n, n_correct], on each
of the step's five kernel paths,

    sw_one_launch   lstm_sw_step_kernel (forward map 5 + BPTT map 4, register dW)
    sw_two_launch   lstm_sw_fwd* maps 0 / 1 / 2 / 5 / 6 / 8, lstm_sw_bwd maps 0-4, lstm_small_dw unless map 4
    one_launch      lstm_small_step_gs_kernel
    deferred_dw     lstm_small_fwd (head epilogue), lstm_small_bwd_dwout, lstm_small_dw
    register_dw     lstm_small_fwd (head epilogue), lstm_small_bwd

all ending in slab_reduce_adam_kernel.  The binding is called directly (no
Trainer, MotionModel or synthetic data); a case selects its path with PDRNN_SW
and PDRNN_TUNE and asserts lstm_head_step_plan's path, wave maps and nb_dw
before the launch.  CASES is the one table of GPU cases; the CPU tests walk
the same table.

Bounds: _head_step_ref.py's docstring derives them (the recurrent budget of
_small_ref.py unchanged, the head's from the per-element bound of h_T).  They
are evaluated on the free-running fp64 reference; test_fp32_reference_run_
stays_in_budget shows on the CPU, for every case of the table, that a plain
fp32 run of the reference meets them and that no row's top-2 logit margin is
within twice the logit bound (apart from the planted exact ties), so the
count of correct predictions is compared exactly.

Every case also checks: flat_grad is a view of exactly P elements inside a
NaN-padded buffer, itself pre-filled with NaN, the result finite and the
padding untouched; a second call gives the same bits; where B T is no
multiple of 16 (the dW kernel's masked tail stage runs) NaN-filled device
blocks are allocated and freed before the call, one large and several below
1 MiB for the caching allocator's two pools, and before the second call also
one of the size of every block the allocator holds free (the first call's
released workspaces among them), so that the step's workspaces (hseq, act,
slab, head slab, xg and their padding rows) are likely to be cut from
non-finite memory.  That part is best effort: the test cannot prove that the
allocator handed those blocks back.

Worst |kernel - ref| / bound per path / map tag and tensor (records, not
thresholds) and the time of the GPU cases, measured on an MI355X when this
file was written:

    deferred_dw gru H16                w_ih 0.000  w_hh 0.001  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    deferred_dw gru H32                w_ih 0.079  w_hh 0.034  b 0.026  head_w 0.068  head_b 0.005  loss 0.001
    deferred_dw gru H64                w_ih 0.000  w_hh 0.002  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    deferred_dw lstm H16               w_ih 0.000  w_hh 0.001  b 0.000  head_w 0.002  head_b 0.003  loss 0.000
    deferred_dw lstm H32               w_ih 0.003  w_hh 0.012  b 0.001  head_w 0.010  head_b 0.003  loss 0.001
    deferred_dw lstm H64               w_ih 0.000  w_hh 0.001  b 0.000  head_w 0.003  head_b 0.002  loss 0.002
    one_launch gru H16                 w_ih 0.002  w_hh 0.003  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    one_launch gru H32                 w_ih 0.015  w_hh 0.007  b 0.008  head_w 0.082  head_b 0.003  loss 0.001
    one_launch lstm H16                w_ih 0.002  w_hh 0.004  b 0.001  head_w 0.003  head_b 0.001  loss 0.002
    one_launch lstm H32                w_ih 0.001  w_hh 0.003  b 0.002  head_w 0.009  head_b 0.002  loss 0.001
    register_dw gru H16 nb1 nbf2       w_ih 0.003  w_hh 0.001  b 0.000  head_w 0.002  head_b 0.001  loss 0.001
    register_dw gru H32 nb1 nbf2       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.001  loss 0.001
    register_dw gru H64 nb1            w_ih 0.004  w_hh 0.002  b 0.002  head_w 0.024  head_b 0.001  loss 0.002
    register_dw lstm H16 nb1 nbf2      w_ih 0.001  w_hh 0.001  b 0.000  head_w 0.002  head_b 0.001  loss 0.001
    register_dw lstm H16 nb2           w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  loss 0.001
    register_dw lstm H32 nb1 nbf2      w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    register_dw lstm H32 nb2           w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.000  loss 0.001
    register_dw lstm H32 nb3           w_ih 0.004  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.001  loss 0.000
    register_dw lstm H64 nb1           w_ih 0.003  w_hh 0.010  b 0.001  head_w 0.030  head_b 0.001  loss 0.001
    sw_one_launch gru H32 f5 b4        w_ih 0.040  w_hh 0.021  b 0.020  head_w 0.064  head_b 0.002  loss 0.001
    sw_one_launch lstm H32 f5 b4       w_ih 0.002  w_hh 0.009  b 0.001  head_w 0.010  head_b 0.002  loss 0.002
    sw_two_launch gru H32 f0 b0        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.001  loss 0.001
    sw_two_launch gru H32 f1 b1        w_ih 0.010  w_hh 0.004  b 0.004  head_w 0.017  head_b 0.001  loss 0.000
    sw_two_launch gru H32 f2 b2        w_ih 0.010  w_hh 0.004  b 0.000  head_w 0.002  head_b 0.001  loss 0.002
    sw_two_launch gru H32 f2 b3        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    sw_two_launch gru H32 f2 b4        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.000  loss 0.000
    sw_two_launch gru H32 f5 b2        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.000  loss 0.000
    sw_two_launch gru H32 f5 b3        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.004  head_b 0.001  loss 0.001
    sw_two_launch gru H32 f5 b4        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.003  loss 0.000
    sw_two_launch gru H32 f6 b2        w_ih 0.026  w_hh 0.037  b 0.027  head_w 0.022  head_b 0.001  loss 0.001
    sw_two_launch gru H32 f6 b3        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.004  loss 0.001
    sw_two_launch gru H32 f6 b4        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    sw_two_launch gru H32 f8 b2        w_ih 0.001  w_hh 0.000  b 0.000  head_w 0.004  head_b 0.001  loss 0.000
    sw_two_launch gru H32 f8 b3        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  loss 0.001
    sw_two_launch gru H32 f8 b4        w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.000  loss 0.000
    sw_two_launch lstm H32 f0 b0       w_ih 0.000  w_hh 0.013  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    sw_two_launch lstm H32 f1 b1       w_ih 0.000  w_hh 0.007  b 0.000  head_w 0.005  head_b 0.001  loss 0.001
    sw_two_launch lstm H32 f2 b2       w_ih 0.010  w_hh 0.030  b 0.000  head_w 0.002  head_b 0.001  loss 0.000
    sw_two_launch lstm H32 f2 b3       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.001  loss 0.002
    sw_two_launch lstm H32 f2 b4       w_ih 0.001  w_hh 0.001  b 0.000  head_w 0.004  head_b 0.000  loss 0.000
    sw_two_launch lstm H32 f5 b2       w_ih 0.000  w_hh 0.001  b 0.000  head_w 0.003  head_b 0.001  loss 0.001
    sw_two_launch lstm H32 f5 b3       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.001  loss 0.001
    sw_two_launch lstm H32 f5 b4       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.002  loss 0.001
    sw_two_launch lstm H32 f6 b2       w_ih 0.003  w_hh 0.009  b 0.003  head_w 0.010  head_b 0.001  loss 0.001
    sw_two_launch lstm H32 f6 b3       w_ih 0.000  w_hh 0.002  b 0.000  head_w 0.003  head_b 0.003  loss 0.001
    sw_two_launch lstm H32 f6 b4       w_ih 0.000  w_hh 0.001  b 0.000  head_w 0.004  head_b 0.000  loss 0.001
    sw_two_launch lstm H32 f8 b2       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  head_b 0.001  loss 0.000
    sw_two_launch lstm H32 f8 b3       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.003  loss 0.001
    sw_two_launch lstm H32 f8 b4       w_ih 0.000  w_hh 0.000  b 0.000  head_w 0.002  head_b 0.000  loss 0.000

The 201 cases of test_step take 1.7 s together (operands and the fp64 reference on the CPU,
two launches, the comparison), the file's 261 GPU tests 3.88 s.
"""
import collections
import dataclasses
import functools
import math
import time
from typing import Optional

import pytest
import torch

import _head_step_ref as HR
import _small_ref as R
from _tune import set_tune

gpu = pytest.mark.gpu
F64 = torch.float64
CELLS = {0: "lstm", 1: "gru"}
PATHS = ("sw_one_launch", "sw_two_launch", "one_launch", "deferred_dw", "register_dw")

_worst = collections.defaultdict(float)  # (tag, tensor) -> worst error / bound
_ran = {}                                # case id -> tag it ran under
_t_gpu = [0.0]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _worst:
        print("\nworst |kernel - ref| / bound per path / map tag and tensor")
        rows = collections.defaultdict(dict)
        for (tag, name), v in _worst.items():
            rows[tag][name] = v
        for tag in sorted(rows):
            print(f"RATIO {tag:34s} " + "  ".join(f"{n} {v:.3f}" for n, v in rows[tag].items()))
        print(f"TIME {len(_ran)} GPU cases of test_step: {_t_gpu[0]:.1f} s")


# ---------------------------------------------------------------------------
# the table of cases
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    path: str
    cell: int
    H: int
    NL: int
    T: int
    B: int
    I: int
    C: int
    hb: bool                      # head bias
    x: str = "direct"             # direct | idx (gathered from a larger table, a row repeated) | bf16
    rbf: bool = False             # round_bf16
    wscale: float = 1.0           # stack weights scaled: gates saturate
    tie: Optional[str] = None     # exact tie of the two largest logits of row 0, the label on the lo | hi class
    fm: int = -1                  # PDRNN_TUNE sw_mode
    bm: int = -1                  # PDRNN_TUNE sw_bwd_mode
    want: tuple = (-1, -1)        # the wave maps the plan must give
    sw_env: Optional[str] = None  # PDRNN_SW
    dwout: Optional[str] = None   # PDRNN_TUNE dwout
    nb_bwd: int = 0               # PDRNN_TUNE nb_bwd
    nb_fwd: int = 0               # PDRNN_TUNE nb_fwd
    seed: int = 0

    @property
    def id(self):
        s = f"{self.path}-{CELLS[self.cell]}-H{self.H}x{self.NL}-T{self.T}-B{self.B}-I{self.I}-C{self.C}"
        s += "b" if self.hb else ""
        if self.path.startswith("sw") and self.path != "sw_one_launch":
            s += f"-m{self.fm}.{self.bm}"
        for flag, text in ((self.x != "direct", self.x), (self.rbf, "rbf"), (self.wscale != 1.0, f"w{self.wscale}"),
                           (self.tie, f"tie{self.tie}"), (self.nb_bwd, f"nbb{self.nb_bwd}"),
                           (self.nb_fwd, f"nbf{self.nb_fwd}")):
            if flag:
                s += "-" + text
        return s

    @property
    def tag(self):
        t = f"{self.path} {CELLS[self.cell]} H{self.H}"
        if self.path.startswith("sw"):
            t += f" f{self.want[0]} b{self.want[1]}"
        if self.path == "register_dw":
            t += f" nb{max(self.nb_bwd, 1)}" + (" nbf2" if self.nb_fwd == 2 else "")
        return t


HEADS = [(6, True), (1, False), (16, True), (2, False), (6, False), (2, True), (16, False), (1, True)]
WSAT = 12.0  # the saturating cases' weight scale (test_fp32_reference_run_stays_in_budget decides how far)


# cases whose first seed leaves a row's top-2 logit margin under twice its logit
# bound (test_fp32_reference_run_stays_in_budget): they take the next one
_NEXT_SEED = {"sw_two_launch-lstm-H32x2-T4-B17-I12-C16-m2.2-idx", "one_launch-gru-H32x2-T4-B17-I9-C16b-idx",
              "deferred_dw-gru-H32x2-T4-B17-I1-C16-idx", "register_dw-gru-H64x1-T7-B5-I4-C2"}


def _cases():
    out = []
    count = collections.Counter()

    def add(path, cell, H, NL, T, B, I=None, **kw):
        n = count[(path, cell)]  # heads, x variants and widths rotate within a path and cell
        count[(path, cell)] += 1
        sw = path.startswith("sw")
        if I is None:  # 1, 4, 9, 12 over the table; the gate-split family also I = H
            I = ((1, 4, 9, 12) if sw else (9, 1, H, 4, 12))[n % (4 if sw else 5)]
        C, hb = kw.pop("head", HEADS[n % len(HEADS)])
        x = kw.pop("x", ("direct", "idx", "bf16")[n % 3])
        if x == "bf16" and cell == 1:
            x = "idx"  # the GRU step takes fp32 x only
        c = Case(path, cell, H, NL, T, B, I, C, hb, x=x, seed=1000 * len(out) + 17 * n + cell, **kw)
        if c.id in _NEXT_SEED:
            c = dataclasses.replace(c, seed=c.seed + 1)
        out.append(c)

    def sw1(cell, T, B, **kw):
        assert T % 4 == 0
        add("sw_one_launch", cell, 32, 2, T, B, want=(5, 4), **kw)

    def sw2(cell, NL, T, B, fm, bm=-1, **kw):
        wf = 6 if fm == 8 and T % 16 else fm
        wb = fm if NL == 1 else (2 if bm == 4 and T % 4 else bm)
        add("sw_two_launch", cell, 32, NL, T, B, fm=fm, bm=bm, want=(wf, wb),
            sw_env="2" if (wf, wb) == (5, 4) else None, **kw)

    def gs1(cell, H, NL, T, B, **kw):
        add("one_launch", cell, H, NL, T, B, sw_env="0", **kw)

    def dd(cell, H, NL, T, B, **kw):
        add("deferred_dw", cell, H, NL, T, B, sw_env="0", dwout="force", **kw)

    def rd(cell, H, NL, T, B, nb_bwd=0, **kw):
        # H = 64 has no one-launch step; below it two or three sequences per
        # backward workgroup (LSTM) or two per forward workgroup rule it out
        nb_fwd = 2 if (H < 64 and nb_bwd == 0) else 0
        add("register_dw", cell, H, NL, T, B, sw_env="0", nb_bwd=nb_bwd, nb_fwd=nb_fwd, **kw)

    for cell in (0, 1):
        # ---- sequence-in-wave, one launch: T % 4 == 0 only
        for T, B in ((4, 1), (4, 5), (16, 2), (16, 3), (20, 5), (20, 1), (8, 2), (12, 5)):
            sw1(cell, T, B)
        sw1(cell, 4, 17, head=(16, True), x="idx")      # every class present
        sw1(cell, 8, 3, wscale=WSAT, head=(6, True))
        sw1(cell, 8, 5, tie="lo", head=(6, True))
        sw1(cell, 8, 5, tie="hi", head=(16, False))
        if cell == 0:
            sw1(cell, 12, 3, rbf=True, x="bf16")
        # ---- sequence-in-wave, two launches, two layers: every forward map
        # with every backward map; T = 5, 7 turn map 4 into 2, T = 20, 33 turn
        # map 8 into 6; B = 5, T = 33: 165 rows, 11 dW stages, 2 chunks, 5 tail rows
        shapes = [(4, 1), (5, 2), (7, 3), (16, 5), (20, 2), (33, 5), (16, 1), (7, 5), (32, 3), (5, 5), (20, 3), (33, 2)]
        n = 0
        for fm in (2, 5, 6, 8):
            for bm in (2, 3, 4):
                for j in range(2):
                    T, B = shapes[(n + 5 * j) % len(shapes)]
                    sw2(cell, 2, T, B, fm, bm)
                    n += 1
        sw2(cell, 2, 16, 3, 8, 4)                        # one chunk of map 8 in front of the register-dW BPTT
        sw2(cell, 2, 32, 5, 8, 3)                        # two chunks
        sw2(cell, 2, 33, 5, 6, 3, x="idx")
        sw2(cell, 2, 4, 17, 2, 2, head=(16, False), x="idx")
        sw2(cell, 2, 7, 3, 6, 2, wscale=WSAT, head=(6, True))
        sw2(cell, 2, 7, 5, 2, 3, tie="lo", head=(6, False))
        sw2(cell, 2, 7, 5, 5, 2, tie="hi", head=(6, True))
        if cell == 0:
            sw2(cell, 2, 7, 3, 6, 3, rbf=True)
        # ---- one layer: a wave runs one (map 0) or two (map 1) sequences
        for fm in (0, 1):
            for T, B in ((4, 1), (7, 3), (33, 5), (16, 2)):
                sw2(cell, 1, T, B, fm)
        sw2(cell, 1, 7, 3, 1, wscale=WSAT, head=(6, True))
        sw2(cell, 1, 5, 5, 1, tie="hi", head=(6, True))
        # ---- gate-split one-launch step: also T = 1, 3, below the dW floor
        for H, NL, T, B in ((16, 1, 1, 1), (16, 2, 3, 2), (32, 1, 4, 3), (32, 2, 5, 5), (16, 4, 7, 1), (32, 3, 16, 2),
                            (16, 2, 20, 3), (32, 2, 33, 5), (32, 2, 1, 5), (16, 1, 3, 3)):
            gs1(cell, H, NL, T, B)
        gs1(cell, 32, 2, 4, 17, head=(16, True), x="idx")
        gs1(cell, 32, 2, 7, 3, wscale=WSAT, head=(6, True))
        gs1(cell, 16, 2, 7, 5, tie="lo", head=(6, True))
        gs1(cell, 32, 1, 7, 5, tie="hi", head=(6, False), I=9)
        if cell == 0:
            gs1(cell, 32, 2, 7, 3, rbf=True, x="bf16")
        # ---- deferred dW (forced: at these batches the plan would not defer)
        for H, NL, T, B in ((16, 1, 4, 1), (16, 2, 5, 2), (32, 1, 7, 3), (32, 2, 16, 5), (64, 1, 20, 1), (64, 1, 33, 5),
                            (32, 2, 33, 5), (16, 4, 7, 5), (64, 1, 4, 2), (32, 4, 5, 3), (64, 1, 7, 3)):
            dd(cell, H, NL, T, B)
        dd(cell, 32, 2, 4, 17, head=(16, False), x="idx")
        dd(cell, 32, 2, 7, 3, wscale=WSAT, head=(6, True))
        dd(cell, 64, 1, 7, 5, tie="lo", head=(6, True))
        dd(cell, 16, 2, 5, 5, tie="hi", head=(16, True))
        if cell == 0:
            dd(cell, 32, 2, 7, 3, rbf=True)
        # ---- register dW: H = 64 as the plan gives it, two sequences per
        # forward workgroup, and (LSTM) two / three per backward workgroup
        for H, NL, T, B, nbb in ((64, 1, 1, 1, 0), (64, 1, 3, 2, 0), (64, 1, 4, 3, 0), (64, 1, 7, 5, 0),
                                 (64, 1, 33, 2, 0), (32, 2, 1, 5, 0), (16, 2, 3, 3, 0), (32, 1, 20, 5, 0),
                                 (16, 4, 7, 2, 0)):
            rd(cell, H, NL, T, B, nbb)
        if cell == 0:
            for H, NL, T, B, nbb in ((32, 2, 3, 5, 2), (32, 2, 7, 3, 3), (32, 1, 20, 5, 3), (32, 2, 33, 5, 2),
                                     (32, 2, 1, 2, 3), (16, 2, 5, 5, 2)):
                rd(cell, H, NL, T, B, nbb)
            rd(cell, 32, 2, 7, 5, 2, rbf=True, x="bf16")
        rd(cell, 64, 1, 4, 17, head=(16, True), x="idx")
        rd(cell, 64, 1, 7, 3, wscale=WSAT, head=(6, True))
        rd(cell, 32, 2, 7, 5, tie="lo", head=(16, True))
        rd(cell, 64, 1, 5, 5, tie="hi", head=(6, False))
    return out


CASES = _cases()
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES), "case ids must be unique"


# ---------------------------------------------------------------------------
# operands and reference of a case (CPU, built once per case)
# ---------------------------------------------------------------------------
class _Operands:
    pass


def _bf16(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _operands(case: Case) -> _Operands:
    """The case's module, head, table, idx and labels on the CPU, and the
    reference results on them (computed once; nothing writes to them)."""
    c = case
    g = torch.Generator().manual_seed(c.seed)
    s = _Operands()
    with torch.no_grad():
        state = torch.random.get_rng_state()
        torch.manual_seed(c.seed)
        s.rnn = (torch.nn.LSTM if c.cell == 0 else torch.nn.GRU)(c.I, c.H, c.NL, batch_first=True)
        torch.random.set_rng_state(state)
        for p in s.rnn.parameters():
            p.mul_(c.wscale)
        k = 1.0 / math.sqrt(c.H)
        s.head_w = (torch.rand(c.C, c.H, generator=g) * 2 - 1) * k
        s.head_b = (torch.rand(c.C, generator=g) * 2 - 1) * k if c.hb else None
        gathered = c.x == "idx"
        N = c.B + 3 if gathered else c.B
        s.x = torch.randn(N, c.T, c.I, generator=g) * 0.5
        if c.x == "bf16":
            s.x = s.x.to(torch.bfloat16)
        s.idx = None
        s.labels = (torch.arange(N) + c.seed) % c.C
        if gathered:
            s.idx = (torch.arange(c.B) * 7) % N   # (7 is coprime with every N = B + 3 of the table)
            s.idx[c.B - 1] = s.idx[0]  # a repeated row
            unused = torch.ones(N, dtype=torch.bool)
            unused[s.idx] = False
            assert bool(unused.any())
            s.x[unused] = float("nan")
            s.labels[unused] = -1      # (int64 has no NaN: a class that matches nothing)
            s.labels[s.idx] = (torch.arange(c.B) + c.seed) % c.C
        s.ws = [getattr(s.rnn, f"{n}_l{l}").detach() for l in range(c.NL)
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        s.ws_ref = [_bf16(w) for w in s.ws] if c.rbf else s.ws  # round_bf16: the reference on the rounded values
        if c.tie:
            # rows lo < hi of the head made identical (weights and bias): their
            # logits are the same bits in every arithmetic.  One of them is row
            # 0's largest logit, so row 0 ties at the top
            assert c.C >= 3
            z = HR.step(s.x.float(), s.idx, s.labels, s.ws_ref, s.head_w, s.head_b, c.cell)["logits"]
            top = int(z[0].argmax())
            other = (top + 1 + c.seed % (c.C - 1)) % c.C
            lo, hi = min(top, other), max(top, other)
            s.head_w[other] = s.head_w[top]
            if s.head_b is not None:
                s.head_b[other] = s.head_b[top]
            s.labels[int(s.idx[0]) if gathered else 0] = lo if c.tie == "lo" else hi
            s.tie = (lo, hi)
        s.ref = HR.step(s.x.float(), s.idx, s.labels, s.ws_ref, s.head_w, s.head_b, c.cell)
    return s


def _segments(offsets):
    """name of a recorded tensor -> list of (start, end) in flat."""
    seg = collections.defaultdict(list)
    for name, span in offsets.items():
        key = "b" if name.startswith("b_") else name.split("_l")[0]
        seg[key].append((name, span))
    return seg


def compare(tag, flat, stats, ref, worst=None):
    """Every element of flat against its budget, the loss against its bound,
    n and n_correct exactly.  Records the worst ratio per (tag, tensor) and
    raises naming every parameter / statistic that misses."""
    bad = []
    assert flat.shape == ref["flat"].shape, (tag, tuple(flat.shape), tuple(ref["flat"].shape))
    flat, stats = flat.detach().cpu(), stats.detach().cpu()
    diff = (flat.double() - ref["flat"]).abs()
    exact = torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf")))
    q = torch.where(ref["budget"] > 0, diff / ref["budget"].clamp_min(1e-300), exact)  # (T = 1: dW_hh is exactly 0)
    q = torch.where(torch.isfinite(flat), q, torch.full_like(q, float("inf")))
    for key, spans in _segments(ref["offsets"]).items():
        ratio = 0.0
        for name, (a, b) in spans:
            r = float(q[a:b].max())
            ratio = max(ratio, r)
            if not r <= 1.0:
                bad.append((name, round(r, 3)))
        if worst is not None:
            worst[(tag, key)] = max(worst[(tag, key)], ratio)
    want = ref["stats"]
    r = abs(float(stats[0]) - float(want[0])) / float(ref["loss_bound"]) if math.isfinite(float(stats[0])) else math.inf
    if worst is not None:
        worst[(tag, "loss")] = max(worst[(tag, "loss")], r)
    if not r <= 1.0:
        bad.append(("loss", round(r, 3)))
    if float(stats[1]) != float(want[1]):
        bad.append(("n", float(stats[1]), float(want[1])))
    if float(stats[2]) != float(want[2]):
        bad.append(("n_correct", float(stats[2]), float(want[2])))
    if bad:
        raise AssertionError(f"{tag}: {bad}")


# ---------------------------------------------------------------------------
# the reference against torch autograd, fp64, CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("C", [1, 6, 16])
@pytest.mark.parametrize("hb", [True, False])
@pytest.mark.parametrize("NL", [1, 2])
@pytest.mark.parametrize("cell", [0, 1])
def test_reference_matches_torch_fp64(cell, NL, hb, C, gathered):
    """fp64 nn.LSTM / nn.GRU + nn.Linear + cross_entropy autograd gives the
    reference's flat gradient (nn.GRU's 3H layout, the order of
    model.parameters()) and statistics to fp64 round-off; the GRU's unpack
    index is the one the fused step passes as grad_colmap."""
    from pytorch_distributed_rnn_amd.ops import gru_fused
    torch.manual_seed(100 * cell + 10 * NL + 2 * hb + C + gathered)
    H, B, T, I = 5, 4, 6, 3
    rnn = (torch.nn.LSTM if cell == 0 else torch.nn.GRU)(I, H, NL, batch_first=True).double()
    fc = torch.nn.Linear(H, C, bias=hb).double()
    N = B + 3 if gathered else B
    x = torch.randn(N, T, I, dtype=F64)
    labels = torch.randint(0, C, (N,))
    idx = torch.tensor([5, 0, 2, 5]) if gathered else None
    xb, yb = HR.gather(x, idx, labels)
    logits = fc(rnn(xb)[0][:, -1])
    loss = torch.nn.functional.cross_entropy(logits, yb)
    loss.backward()
    want = torch.cat([p.grad.reshape(-1) for p in list(rnn.parameters()) + list(fc.parameters())])
    with torch.no_grad():
        ws = [getattr(rnn, f"{n}_l{l}") for l in range(NL) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        ref = HR.step(x, idx, labels, ws, fc.weight, fc.bias, cell)
    torch.testing.assert_close(ref["flat"], want, rtol=0, atol=1e-12)
    assert ref["budget"].shape == want.shape and bool((ref["budget"] > 0).all()) and float(ref["loss_bound"]) > 0
    torch.testing.assert_close(ref["stats"][0], loss.detach(), rtol=0, atol=1e-12)
    assert float(ref["stats"][1]) == B
    assert float(ref["stats"][2]) == float((logits.argmax(1) == yb).sum())
    assert ref["offsets"]["head_w"] == (want.numel() - C * H - (C if hb else 0), want.numel() - (C if hb else 0))
    if cell == 1:
        in_dims = tuple([I] + [H] * (NL - 1))
        assert torch.equal(HR.unpack_gru_index(H, in_dims), gru_fused._unpack_index(H, in_dims, torch.device("cpu")))
        for a, b in zip(HR.pack_gru(ws, NL, H), gru_fused._pack(ws, NL, H, x)):
            assert torch.equal(a, b)


def test_lowest_argmax_on_ties():
    z = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 2.0, 2.0]], dtype=F64)
    assert HR.lowest_argmax(z).tolist() == [1, 0, 2] == z.argmax(1).tolist()
    assert HR.top2_margin(z).tolist() == [1.0, math.inf, 1.0]


# ---------------------------------------------------------------------------
# the bound is attainable: every GPU case, fp32 reference run against fp64 (CPU)
# ---------------------------------------------------------------------------
ADAM = dict(lr=2.5e-3, b1=0.8, b2=0.95, eps=1e-6, wd=0.05)


def _adam_state(P, seed):
    """Parameters and moments of a run under way (exp_avg_sq well above the
    gradient's rounding level: from zero moments Adam's first step is
    sign(g) lr, which no gradient bound carries over to the parameters)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(P, generator=g) * 0.3, torch.randn(P, generator=g) * 0.05,
            (0.1 + torch.rand(P, generator=g)) ** 2 * 0.1)


def _adam_close(got_p, ref_p):
    """The bound of tests/test_gpu_adam.py for the folded kernel's parameters."""
    got_p, ref_p = got_p.detach().double().cpu(), ref_p.double()
    return float(((got_p - ref_p).abs() / (1e-6 + 1e-5 * ref_p.abs())).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_fp32_reference_run_stays_in_budget(case):
    """What makes the free-running comparison legitimate: on this case's very
    inputs a plain fp32 run of the reference (CPU) is within every budget of
    the fp64 run, its statistics agree, no row's top-2 margin is under twice
    its logit bound unless it is the planted tie, and an Adam step from the
    fp32 gradient lands within the folded kernel's parameter bound."""
    s = _operands(case)
    ref = s.ref
    run32 = HR.step(s.x.float(), s.idx, s.labels, s.ws_ref, s.head_w, s.head_b, case.cell, dtype=torch.float32)
    compare("cpu fp32", run32["flat"], run32["stats"], ref)
    assert bool(torch.isfinite(ref["flat"]).all())
    assert (float(ref["flat"].abs().max()) > 0) == (case.C > 1)  # one class: softmax = onehot, no gradient at all
    margin = HR.top2_margin(ref["logits"])
    need = 2 * ref["ez"].max(1).values
    assert bool((margin >= need).all()), (margin, need)
    z = ref["logits"]
    tied = (z == z.max(1, keepdim=True).values).sum(1) > 1
    if case.tie:
        lo, hi = s.tie
        assert bool(tied[0]) and float(z[0, lo]) == float(z[0].max()) and bool((z[:, lo] == z[:, hi]).all())
        assert bool((run32["logits"][:, lo] == run32["logits"][:, hi]).all())
        yb = HR.gather(s.x, s.idx, s.labels)[1]
        assert int(yb[0]) == (lo if case.tie == "lo" else hi)
    else:
        assert case.C == 1 or not bool(tied.any())
    P = ref["flat"].numel()
    p, m, v = _adam_state(P, case.seed)
    hp = (ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], 3.0, True)
    assert _adam_close(HR.adam_step(p, run32["flat"], m, v, *hp)[0], HR.adam_step(p, ref["flat"], m, v, *hp)[0]) <= 1.0
    if case.wscale != 1.0:  # the gates do saturate
        sat = R.forward(HR.gather(s.x.float(), s.idx, s.labels)[0], HR.pack_gru(s.ws_ref, case.NL, case.H)
                        if case.cell == 1 else s.ws_ref, None, None, case.H, case.NL, case.cell)[1][:, :, :, :2]
        assert float(((sat < 0.02) | (sat > 0.98)).double().mean()) > 0.1


def test_every_class_present_somewhere():
    """Cases whose batch holds every class of the head, per path."""
    for path in PATHS:
        full = [c for c in CASES if c.path == path and c.C > 2 and
                len(set(HR.gather(_operands(c).x, _operands(c).idx, _operands(c).labels)[1].tolist())) == c.C]
        assert full, path


# ---------------------------------------------------------------------------
# the comparison rejects planted defects (CPU)
# ---------------------------------------------------------------------------
def _defect_inputs(cell, tie=False):
    torch.manual_seed(7 + cell)
    H, NL, B, T, I, C = 8, 2, 5, 7, 3, 6   # B T = 35: 3 rows past the last whole 16-row stage
    k = 1.0 / math.sqrt(H)
    G = 4 if cell == 0 else 3
    ws = []
    for l in range(NL):
        Il = I if l == 0 else H
        ws += [(torch.rand(G * H, Il) * 2 - 1) * k, (torch.rand(G * H, H) * 2 - 1) * k,
               (torch.rand(G * H) * 2 - 1) * k, (torch.rand(G * H) * 2 - 1) * k]
    head_w, head_b = (torch.rand(C, H) * 2 - 1) * 2 * k, (torch.rand(C) * 2 - 1) * k
    x = torch.randn(B, T, I)
    labels = torch.arange(B) % C
    if tie:
        z = HR.step(x, None, labels, ws, head_w, head_b, cell)["logits"]
        top = int(z[0].argmax())
        other = (top + 2) % C
        head_w[other], head_b[other] = head_w[top], head_b[top]
        labels[0] = max(top, other)
    return dict(x=x, labels=labels, ws=ws, head_w=head_w, head_b=head_b, cell=cell, H=H, NL=NL, B=B, T=T, I=I, C=C)


def _defect(kind, a, ref):
    """(flat, stats): the fp64 reference rounded to fp32, with one defect."""
    flat, stats = ref["flat"].clone(), ref["stats"].clone()
    H, NL, B, T, I, C, cell = a["H"], a["NL"], a["B"], a["T"], a["I"], a["C"], a["cell"]
    off = ref["offsets"]
    w4 = HR.pack_gru(a["ws"], NL, H) if cell == 1 else a["ws"]
    x = a["x"].double()
    hseq, act, hn, _ = R.forward(x, w4, None, None, H, NL, cell)
    z = ref["logits"]
    onehot = torch.nn.functional.one_hot(a["labels"], C).double()
    d = (torch.softmax(z, 1) - onehot) / B
    dhn = hseq.new_zeros(NL, B, H)
    dhn[NL - 1] = d @ a["head_w"].double()
    dg = R.gate_grads(w4, None, None, hseq, act, None, dhn, None, H, NL, cell)[0]
    G = 4 if cell == 0 else 3

    def seg(name):
        s, e = off[name]
        return flat[s:e]

    if kind == "h_prev at t = 0 not masked in dW_hh":
        # the row in front of (b, 0) in the [B T, H] stream: the sequence before's h_{T-1}
        before = torch.cat([hseq.new_ones(1, H), hseq[0, :-1, -1]])
        assert cell == 0
        seg("w_hh_l0").add_((dg[0, :, 0].t() @ before).reshape(-1))
    elif kind == "one sequence's contribution missing":
        assert cell == 0
        rnn = R.param_grads(dg, x, None, hseq, True, rows=slice(0, B - 1))[0]
        flat[:rnn.numel()] = rnn
        seg("head_w").copy_((d[:-1].t() @ hn[NL - 1][:-1]).reshape(-1))
        seg("head_b").copy_(d[:-1].sum(0))
        stats[0] -= (torch.logsumexp(z, 1) - (z * onehot).sum(1))[-1] / B
    elif kind == "last B T % 16 rows missing from one layer's dW":
        r = B * T % 16
        assert r and cell == 0
        g, hin = dg[1].reshape(B * T, -1)[:-r], hseq[0].reshape(B * T, -1)[:-r]
        seg("w_ih_l1").copy_((g.t() @ hin).reshape(-1))
    elif kind == "db_ih != db_hh":
        seg("b_hh_l0").mul_(0.5)
    elif kind == "head db not divided by B":
        seg("head_b").mul_(B)
    elif kind == "loss as sum instead of mean":
        stats[0] *= B
    elif kind == "a tie counted for the higher class":
        pred = (C - 1) - z.flip(1).argmax(1)  # the highest index among equal logits
        stats[2] = float((pred == a["labels"]).sum())
        assert stats[2] != ref["stats"][2]
    elif kind == "a GRU zero-block column landing in flat":
        # grad_colmap one block off for layer 0's n rows of W_ih: the gradient of the packed zero block (n_h rows)
        assert cell == 1
        packed = (dg[0].reshape(B * T, -1).t() @ x.reshape(B * T, -1))  # [4H, I]
        seg("w_ih_l0").view(3 * H, I)[2 * H:].copy_(packed[3 * H:])
    elif kind == "an x column >= I contributing to dW_ih":
        # column I of the zero-padded x image holds 1 instead of 0 and its tile
        # column is stored: it lands on element (r + 1, 0) of the [G H, I] gradient
        extra = dg[0].reshape(B * T, -1)[:, :G * H].sum(0)
        seg("w_ih_l0").view(G * H, I)[1:, 0].add_(extra[:G * H - 1])
    else:
        raise KeyError(kind)
    return flat.float(), stats.float()


_DEFECTS = [("h_prev at t = 0 not masked in dW_hh", 0, "w_hh_l0"), ("one sequence's contribution missing", 0, "head_w"),
            ("last B T % 16 rows missing from one layer's dW", 0, "w_ih_l1"), ("db_ih != db_hh", 0, "b_hh_l0"),
            ("db_ih != db_hh", 1, "b_hh_l0"), ("head db not divided by B", 0, "head_b"),
            ("loss as sum instead of mean", 1, "loss"), ("a tie counted for the higher class", 0, "n_correct"),
            ("a GRU zero-block column landing in flat", 1, "w_ih_l0"),
            ("an x column >= I contributing to dW_ih", 0, "w_ih_l0"),
            ("an x column >= I contributing to dW_ih", 1, "w_ih_l0")]


@pytest.mark.parametrize("cell,tie", [(0, False), (1, False), (0, True)])
def test_comparison_accepts_rounded_reference(cell, tie):
    a = _defect_inputs(cell, tie)
    ref = HR.step(a["x"], None, a["labels"], a["ws"], a["head_w"], a["head_b"], cell)
    compare("cpu", ref["flat"].float(), ref["stats"].float(), ref)


@pytest.mark.parametrize("kind,cell,named", _DEFECTS, ids=[f"{k}-{CELLS[c]}" for k, c, _ in _DEFECTS])
def test_comparison_rejects_defect(kind, cell, named):
    """Each planted defect fails the comparison that the undamaged fp32 copy
    passes, and the failure names the damaged parameter or statistic."""
    a = _defect_inputs(cell, tie=kind.startswith("a tie"))
    ref = HR.step(a["x"], None, a["labels"], a["ws"], a["head_w"], a["head_b"], cell)
    flat, stats = _defect(kind, a, ref)
    with pytest.raises(AssertionError) as e:
        compare("cpu", flat, stats, ref)
    assert f"'{named}'" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------
# the kernels against the reference
# ---------------------------------------------------------------------------
def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.require()


class _Call:
    """A case's device operands and the arguments of the binding."""

    def __init__(self, case, monkeypatch):
        from pytorch_distributed_rnn_amd.ops import gru_fused
        from pytorch_distributed_rnn_amd.ops.lstm import LSTM, step_launch_config
        c, s = case, _operands(case)
        self.case, self.s, self.mod = c, s, _mod()
        dev = torch.device("cuda")
        # ---- the path: PDRNN_SW and PDRNN_TUNE, then what the plan makes of them
        if c.sw_env is None:
            monkeypatch.delenv("PDRNN_SW", raising=False)
        else:
            monkeypatch.setenv("PDRNN_SW", c.sw_env)
        set_tune(monkeypatch, dwout=c.dwout, dwout_nb=None, split_fwd=None, split_bwd=None,
                 sw_mode=str(c.fm) if c.fm >= 0 else None, sw_bwd_mode=str(c.bm) if c.bm >= 0 else None,
                 nb_bwd=str(c.nb_bwd) if c.nb_bwd else None, nb_fwd=str(c.nb_fwd) if c.nb_fwd else None)
        # (the LSTM's config for either cell: the table pins what differs through PDRNN_TUNE)
        (self.nb_fwd, self.sp_fwd), self.nb_bwd = step_launch_config(LSTM, c.B, c.H, c.NL)
        assert (self.nb_fwd, self.nb_bwd) == (max(c.nb_fwd, 1), max(c.nb_bwd, 1))
        plan = self.mod.lstm_head_step_plan(c.H, c.I, c.NL, c.T, c.B, cell=c.cell, nb_fwd=self.nb_fwd,
                                            split_fwd=self.sp_fwd, nb_bwd=self.nb_bwd, split_bwd=0)
        self.plan = plan
        assert plan["path"] == c.path, (c.id, plan)
        if c.path.startswith("sw"):
            assert (plan["sw_fmode"], plan["sw_bmode"]) == c.want, (c.id, plan)
        else:
            assert not plan["sw"], (c.id, plan)
        assert plan["nb_dw"] == (self.nb_bwd if c.path == "register_dw" else 1), (c.id, plan)
        if c.path == "register_dw" and c.cell == 0:
            assert plan["nb_bwd"] == self.nb_bwd
        # ---- operands
        rnn = (torch.nn.LSTM if c.cell == 0 else torch.nn.GRU)(c.I, c.H, c.NL, batch_first=True)
        rnn.load_state_dict(s.rnn.state_dict())
        rnn = rnn.cuda()
        ws = [getattr(rnn, f"{n}_l{l}").detach() for l in range(c.NL)
              for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        self.colmap = None
        if c.cell == 1:
            in_dims = tuple(int(ws[4 * l].shape[1]) for l in range(c.NL))
            self.colmap = gru_fused._unpack_index(c.H, in_dims, dev).to(torch.int32)
            ws = gru_fused._pack(ws, c.NL, c.H, ws[0])
        self.ws = ws
        self.x, self.labels = s.x.to(dev), s.labels.to(dev)
        self.idx = s.idx.to(dev) if s.idx is not None else None
        self.head_w = s.head_w.to(dev)
        self.head_b = s.head_b.to(dev) if s.head_b is not None else None
        self.P = s.ref["flat"].numel()
        self.new_buffers()

    def new_buffers(self):
        """flat_grad: P elements at an odd offset of a NaN buffer, NaN itself;
        stats likewise."""
        self.buf = torch.full((self.P + 77,), float("nan"), device="cuda")
        self.flat = self.buf[33:33 + self.P]
        self.sbuf = torch.full((9,), float("nan"), device="cuda")
        self.stats = self.sbuf[3:6]

    def __call__(self, stats=None, **kw):
        c = self.case
        self.mod.lstm_head_train_step(self.x, self.idx, self.labels, self.ws, self.head_w, self.head_b, self.flat,
                                      self.stats if stats is None else stats, c.H, c.NL, self.sp_fwd, 0, self.nb_fwd,
                                      self.nb_bwd, cell=c.cell, grad_colmap=self.colmap, round_bf16=c.rbf, **kw)

    def padding_untouched(self):
        return bool(torch.isnan(self.buf[:33]).all()) and bool(torch.isnan(self.buf[33 + self.P:]).all()) and \
            bool(torch.isnan(self.sbuf[:3]).all()) and bool(torch.isnan(self.sbuf[6:]).all())


def _poison_allocator(cached=False):
    """NaN-filled blocks handed back to the caching allocator: one large, and
    several below 1 MiB (its small pool), so that the next at::empty of the
    step is likely to be cut from them.  ``cached``: also one block of the
    size of every block the allocator holds free (up to 64 MiB each, 512 MiB
    in all) -- after a first call those include the workspaces it released,
    which the best-fit search hands out again for the same sizes."""
    nan = float("nan")
    blocks = [torch.full((8 << 20,), nan, device="cuda")]
    blocks += [torch.full((n,), nan, device="cuda") for n in (128, 1024, 8192, 65536, 130000, 250000, 250000)]
    if cached:
        torch.cuda.synchronize()
        free = sorted((b["size"] for seg in torch.cuda.memory_snapshot() for b in seg["blocks"]
                       if b["state"] == "inactive" and b["size"] <= 64 << 20), reverse=True)
        total = 0
        for n in free:
            total += n
            if total > 512 << 20:
                break
            blocks.append(torch.full((n // 4,), nan, device="cuda"))
    torch.cuda.synchronize()
    del blocks


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_step(case, monkeypatch):
    t0 = time.perf_counter()
    call = _Call(case, monkeypatch)
    ref = call.s.ref
    if case.B * case.T % 16:
        _poison_allocator()
    call()
    torch.cuda.synchronize()
    flat, stats = call.flat.clone(), call.stats.clone()
    assert call.padding_untouched(), "written outside flat_grad / stats"
    assert bool(torch.isfinite(flat).all()) and bool(torch.isfinite(stats).all())
    compare(case.tag, flat, stats, ref, worst=_worst)
    call.new_buffers()
    if case.B * case.T % 16:
        _poison_allocator(cached=True)  # the workspaces the first call released among them
    call()
    torch.cuda.synchronize()
    assert call.padding_untouched(), "written outside flat_grad / stats"
    assert torch.equal(call.flat, flat) and torch.equal(call.stats, stats), "the step is not deterministic"
    _ran[case.id] = case.tag
    _t_gpu[0] += time.perf_counter() - t0


def _one_per_path(cell=None, pred=lambda c: True):
    out = []
    for path in PATHS:
        for cl in ((0, 1) if cell is None else (cell,)):
            out.append(next(c for c in CASES if c.path == path and c.cell == cl and c.B > 1 and c.T >= 4 and
                            c.wscale == 1.0 and not c.tie and pred(c)))
    return out


@gpu
@pytest.mark.parametrize("step,offset,rows,row", [(3.0, 3, 5, 1), (1.0, -3, 5, 3), (7.9, 0, 8, 7), (4.0, -4, 3, 0)])
@pytest.mark.parametrize("case", _one_per_path(0), ids=lambda c: c.id)
def test_stats_ring_row(case, step, offset, rows, row, monkeypatch):
    """stats_slot_step: the statistics land in row (int(step) + offset) mod
    rows of the [rows, 3] ring (wrapped, negative offset, truncated step) and
    every other row keeps its sentinel."""
    call = _Call(case, monkeypatch)
    assert (int(step) + offset) % rows == row
    ring = torch.full((rows, 3), -7.25, device="cuda")
    step_t = torch.tensor(step, device="cuda")
    call(stats=ring, stats_slot_step=step_t, stats_slot_offset=offset)
    torch.cuda.synchronize()
    compare("ring", call.flat, ring[row], call.s.ref)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[row] = False
    assert bool((ring.cpu()[keep] == -7.25).all()), ring
    assert float(step_t) == float(torch.tensor(step))  # (no device step count without adam_ticket: unchanged)


@gpu
@pytest.mark.parametrize("device_step", [False, True])
@pytest.mark.parametrize("case", _one_per_path(), ids=lambda c: c.id)
def test_folded_adam(case, device_step, monkeypatch):
    """adam_state / adam_hp: the parameters equal a plain fp64 Adam step from
    the REFERENCE gradient within tests/test_gpu_adam.py's bound for the folded
    kernel (rtol 1e-5, atol 1e-6), flat_grad still holds the gradient; with
    adam_ticket the device step count names the step, advances by exactly 1
    per call and the ticket word returns to 0."""
    call = _Call(case, monkeypatch)
    ref = call.s.ref
    p0, m0, v0 = _adam_state(call.P, case.seed)
    hp = [ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], 3.0, 1.0]
    p, m, v = p0, m0, v0
    state = [t.cuda() for t in (p0, m0, v0)]
    kw, step_t, ticket, ring = {}, None, None, None
    if device_step:
        step_t = torch.tensor(2.0, device="cuda")      # the count BEFORE the step
        ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
        ring = torch.full((4, 3), -7.25, device="cuda")
        hp[5] = 999.0                                  # the host's count is not the one used
        kw = dict(stats=ring, stats_slot_step=step_t, stats_slot_offset=0, adam_ticket=ticket)
    for k in range(2):
        call.new_buffers()
        if not device_step:
            hp[5] = 3.0 + k
        call(adam_state=state, adam_hp=hp, **kw)
        torch.cuda.synchronize()
        p, m, v = HR.adam_step(p, ref["flat"], m, v, *hp[:5], 3.0 + k, True)
        compare("adam", call.flat, ring[(2 + k) % 4] if device_step else call.stats, ref)
        assert call.padding_untouched()
        r = _adam_close(state[0], p)
        assert r <= 1.0, f"parameters after step {k + 1}: {r:.3f} x (rtol 1e-5, atol 1e-6)"
        if device_step:
            assert float(step_t) == 3.0 + k and int(ticket) == 0
    assert float((state[0].cpu() - p0).abs().max()) > 1e-4


# ---------------------------------------------------------------------------
# refusals: every one a TORCH_CHECK of the binding ahead of its first launch
# ---------------------------------------------------------------------------
_REFUSALS = ["idx on the host", "idx int32", "idx not contiguous", "labels on the host", "labels short",
             "labels short of the table", "labels int32", "head_w on the host", "head_w fp64", "head_b on the host",
             "head_b fp64", "head_b of C + 1", "flat_grad on the host", "flat_grad of P + 1", "stats on the host",
             "C = 17", "stack without biases", "GRU without grad_colmap", "adam_ticket without stats_slot_step"]


@gpu
@pytest.mark.parametrize("what", _REFUSALS)
def test_refusals(what, monkeypatch):
    """Arguments the binding rejects before any launch raise, leave flat_grad
    and stats untouched, and the valid call of the same operands afterwards
    passes."""
    gathered = "idx" in what or "table" in what
    cell = 1 if what.startswith("GRU") else 0
    case = next(c for c in CASES if c.cell == cell and c.hb and c.C > 1 and (c.x == "idx") == gathered and c.B > 1 and
                not c.tie and not c.rbf and c.wscale == 1.0)
    call = _Call(case, monkeypatch)
    good = dict(x=call.x, idx=call.idx, labels=call.labels, ws=call.ws, head_w=call.head_w, head_b=call.head_b,
                flat=call.flat, stats=call.stats, colmap=call.colmap, kw={})
    a = dict(good)
    dev = call.x.device
    if what == "idx on the host":
        a["idx"] = call.idx.cpu()
    elif what == "idx int32":
        a["idx"] = call.idx.int()
    elif what == "idx not contiguous":
        a["idx"] = torch.stack([call.idx, call.idx], 1)[:, 0]
        assert not a["idx"].is_contiguous()
    elif what == "labels on the host":
        a["labels"] = call.labels.cpu()
    elif what == "labels short":
        a["labels"] = call.labels[:-1].contiguous()
    elif what == "labels short of the table":
        a["labels"] = call.labels[:-1].contiguous()
    elif what == "labels int32":
        a["labels"] = call.labels.int()
    elif what == "head_w on the host":
        a["head_w"] = call.head_w.cpu()
    elif what == "head_w fp64":
        a["head_w"] = call.head_w.double()
    elif what == "head_b on the host":
        a["head_b"] = call.head_b.cpu()
    elif what == "head_b fp64":
        a["head_b"] = call.head_b.double()
    elif what == "head_b of C + 1":
        a["head_b"] = torch.zeros(case.C + 1, device=dev)
    elif what == "flat_grad on the host":
        a["flat"] = torch.zeros(call.P)
    elif what == "flat_grad of P + 1":
        a["flat"] = call.buf[33:34 + call.P]
    elif what == "stats on the host":
        a["stats"] = torch.zeros(3)
    elif what == "C = 17":
        a["head_w"], a["head_b"] = torch.zeros(17, case.H, device=dev), torch.zeros(17, device=dev)
        a["flat"] = torch.zeros(call.P + (17 - case.C) * (case.H + 1), device=dev)
    elif what == "stack without biases":
        a["ws"] = [w for j, w in enumerate(call.ws) if j % 4 < 2]
    elif what == "GRU without grad_colmap":
        a["colmap"] = None
    elif what == "adam_ticket without stats_slot_step":
        state = [t.cuda() for t in _adam_state(call.P, 1)]
        a["kw"] = dict(adam_state=state, adam_hp=[2.5e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.0],
                       adam_ticket=torch.zeros(1, dtype=torch.int32, device=dev))
    else:
        raise KeyError(what)

    def run(v):
        call.mod.lstm_head_train_step(v["x"], v["idx"], v["labels"], v["ws"], v["head_w"], v["head_b"], v["flat"],
                                      v["stats"], case.H, case.NL, call.sp_fwd, 0, call.nb_fwd, call.nb_bwd, cell=cell,
                                      grad_colmap=v["colmap"], **v["kw"])
    with pytest.raises(RuntimeError):
        run(a)
    torch.cuda.synchronize()
    assert bool(torch.isnan(call.buf).all()) and bool(torch.isnan(call.sbuf).all()), "a refused call wrote its outputs"
    run(good)
    torch.cuda.synchronize()
    compare("refusal, then valid", call.flat, call.stats, call.s.ref)


# ---------------------------------------------------------------------------
# what ran
# ---------------------------------------------------------------------------
def _expected_tags():
    return {c.id: c.tag for c in CASES}


def test_case_table_covers_every_path_map_and_width():
    """The table itself (no GPU): every path with both cells, every wave map
    kMaps serves (forward 0 1 2 5 6 8, backward 0 1 2 3 4), H = 16 / 32 / 64,
    every T, B, I, head and input variant the kernels branch on."""
    tags = set(_expected_tags().values())
    for path in PATHS:
        for cell in CELLS.values():
            assert any(t.startswith(f"{path} {cell} ") for t in tags), (path, cell)
    sw = [c for c in CASES if c.path.startswith("sw")]
    for cell in (0, 1):
        assert {c.want[0] for c in sw if c.cell == cell} == {0, 1, 2, 5, 6, 8}
        assert {c.want[1] for c in sw if c.cell == cell} == {0, 1, 2, 3, 4}
        assert {c.want for c in sw if c.cell == cell and c.NL == 2} == {(f, b) for f in (2, 5, 6, 8) for b in (2, 3, 4)}
        for path, hs in (("one_launch", {16, 32}), ("deferred_dw", {16, 32, 64}), ("register_dw", {16, 32, 64})):
            assert {c.H for c in CASES if c.path == path and c.cell == cell} == hs, path
        assert {c.T for c in CASES if c.cell == cell} >= {1, 3, 4, 5, 7, 16, 20, 33}
        assert {c.B for c in CASES if c.cell == cell} >= {1, 2, 3, 5}
        for path in PATHS:
            mine = [c for c in CASES if c.path == path and c.cell == cell]
            assert {(c.C, c.hb) for c in mine} == set(HEADS), path
            assert {c.tie for c in mine} == {None, "lo", "hi"}, path
            assert {c.x for c in mine} >= ({"direct", "idx", "bf16"} if cell == 0 else {"direct", "idx"}), path
            assert any(c.wscale != 1.0 for c in mine) and (cell == 1 or any(c.rbf for c in mine)), path
            assert {c.I for c in mine} >= {1, 4, 9, 12}, path
            assert path.startswith("sw") or any(c.I == c.H for c in mine), path
            assert any(c.B * c.T % 16 and c.B * c.T > 64 for c in mine), path
    assert {c.nb_bwd for c in CASES if c.path == "register_dw" and c.H == 32} >= {2, 3}
    assert any(c.B == 5 and c.T == 33 for c in CASES if c.path in ("sw_two_launch", "deferred_dw"))


@gpu
def test_tags_that_ran(monkeypatch):
    """Every case of the table still reaches the path, maps and width its tag
    names: the plan is asked again for each (a host query, no launch), and
    when test_step ran over the whole table in this process the tags it
    recorded are the same set.  A plan change that reroutes a case fails here
    and in that case's own assertion."""
    mod = _mod()
    from pytorch_distributed_rnn_amd.ops.lstm import LSTM, step_launch_config
    seen = set()
    for c in CASES:
        if c.sw_env is None:
            monkeypatch.delenv("PDRNN_SW", raising=False)
        else:
            monkeypatch.setenv("PDRNN_SW", c.sw_env)
        set_tune(monkeypatch, dwout=c.dwout, dwout_nb=None, split_fwd=None, split_bwd=None,
                 sw_mode=str(c.fm) if c.fm >= 0 else None, sw_bwd_mode=str(c.bm) if c.bm >= 0 else None,
                 nb_bwd=str(c.nb_bwd) if c.nb_bwd else None, nb_fwd=str(c.nb_fwd) if c.nb_fwd else None)
        (nb_fwd, sp_fwd), nb_bwd = step_launch_config(LSTM, c.B, c.H, c.NL)
        p = mod.lstm_head_step_plan(c.H, c.I, c.NL, c.T, c.B, cell=c.cell, nb_fwd=nb_fwd, split_fwd=sp_fwd,
                                    nb_bwd=nb_bwd, split_bwd=0)
        tag = f"{p['path']} {CELLS[c.cell]} H{c.H}"
        if p["sw"]:
            tag += f" f{p['sw_fmode']} b{p['sw_bmode']}"
        if p["path"] == "register_dw":
            tag += f" nb{p['nb_dw']}" + (" nbf2" if p["nb_fwd"] == 2 else "")
        assert tag == c.tag, (c.id, p)
        seen.add(tag)
    want = set(_expected_tags().values())
    assert seen == want
    for path in PATHS:
        assert any(t.startswith(path + " ") for t in seen), path
    for f in (0, 1, 2, 5, 6, 8):
        assert any(f" f{f} " in t for t in seen), f
    for b in (0, 1, 2, 3, 4):
        assert any(t.endswith(f" b{b}") for t in seen), b
    for H in (16, 32, 64):
        assert any(f" H{H}" in t for t in seen), H
    if len(_ran) == len(CASES):
        assert set(_ran.values()) == want and _ran == _expected_tags()
