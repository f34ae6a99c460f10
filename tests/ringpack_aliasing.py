"""Operand identity at the entry points of include/hering_ringpack.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  Two outputs never coincide and inputs may coincide
with inputs; the only output-on-input form is out_k == in_k in the sum_only expand step (listed here, refused in the other form);
the pack steps work in place on a / b by definition, and any handle occurring twice among their operands is refused."""
from tests.aliasing_table import ACC, IN, OUT, Q, Row

_CT = {"in0": (IN, Q), "in1": (IN, Q)}

ROWS = {
    "he_ring_split_ntt": Row("he_ring_split_ntt", {"in": (IN, Q), "outEven": (OUT, Q), "outOdd": (OUT, Q)},
                             "rlwe.SplitNTT(ringLarge, level, in, outEven, outOdd)",
                             oracle="NTT_n(INTT_N(in)[0::2]), NTT_n(INTT_N(in)[1::2])"),
    "he_ring_merge_ntt": Row("he_ring_merge_ntt", {"inEven": (IN, Q), "inOdd": (IN, Q), "out": (OUT, Q)},
                             "rlwe.MergeNTT(ringLarge, level, inEven, inOdd, out)",
                             oracle="repeat(inEven, 2) + repeat(inOdd, 2) * XPow2NTT[0]"),
    "he_ringpack_split": Row("he_ringpack_split", {**_CT, "even0": (OUT, Q), "even1": (OUT, Q), "odd0": (OUT, Q), "odd1": (OUT, Q)},
                             "rlwe.RingPackingEvaluator.Split(level, ctN, ctEvenNHalf, ctOddNHalf)",
                             oracle="tests.ringpack_ref.RingPackingEvaluator.Split"),
    "he_ringpack_merge": Row("he_ringpack_merge", {"even0": (IN, Q), "even1": (IN, Q), "odd0": (IN, Q), "odd1": (IN, Q),
                                                    "out0": (OUT, Q), "out1": (OUT, Q)},
                             "rlwe.RingPackingEvaluator.Merge(level, ctEvenNHalf, ctOddNHalf, ctN)",
                             oracle="tests.ringpack_ref.RingPackingEvaluator.Merge"),
    "he_ringpack_expand_step": Row("he_ringpack_expand_step", {**_CT, "tmp0": (IN, Q), "tmp1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)},
                                   "he_ringpack_expand_step(ring, level, k, sum_only, ...)", {("out0", "in0"), ("out1", "in1")},
                                   oracle="out[e] = in[e] + tmp[e]; out[e + m] = (in[e] - tmp[e]) * XInvPow2NTT[k] (sum_only: the first)"),
    "he_ringpack_pack_pre": Row("he_ringpack_pack_pre", {"a0": (ACC, Q), "a1": (ACC, Q), "b0": (ACC, Q), "b1": (ACC, Q),
                                                          "t0": (OUT, Q), "t1": (OUT, Q)},
                                "he_ringpack_pack_pre(ring, level, k, count, a0, a1, b0, b1, t0, t1)",
                                oracle="T = a - b x, a += b x | T = a | b = b x, T = b x", arrays=("a0", "a1", "b0", "b1")),
    "he_ringpack_pack_post": Row("he_ringpack_pack_post", {"a0": (ACC, Q), "a1": (ACC, Q), "b0": (ACC, Q), "b1": (ACC, Q),
                                                            "t0": (IN, Q), "t1": (IN, Q)},
                                 "he_ringpack_pack_post(ring, level, count, a0, a1, b0, b1, t0, t1)",
                                 oracle="a += T | b -= T", arrays=("a0", "a1", "b0", "b1")),
}
