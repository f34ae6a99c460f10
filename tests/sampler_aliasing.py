"""Operand identity at the entry points of include/hering_sampler.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  A sampler entry reads no polynomial but the one it
writes (ReadAndAdd accumulates into it), so the only pair of polynomial operands is (pol, polP) of the ringqp uniform form: two
outputs, never one handle."""
from tests.aliasing_table import OUT, P, Q, Row

ROWS = {
    "he_sampler_uniform_read": Row("he_sampler_uniform_read", {"pol": (OUT, Q), "polP": (OUT, P)},
                                   "sampling.UniformSampler(prng, ringQ, ringP).Read((q, p))", set(),
                                   oracle="tests/sampler_ref.uniform_read_qp on the same stream"),
    "he_sampler_gaussian_read": Row("he_sampler_gaussian_read", {"pol": (OUT, Q)}, "sampling.GaussianSampler(...).Read(pol)", set(),
                                    oracle="tests/sampler_ref.gaussian_read on the same stream"),
    "he_sampler_ternary_read": Row("he_sampler_ternary_read", {"pol": (OUT, Q)}, "sampling.TernarySampler(...).Read(pol)", set(),
                                   oracle="tests/sampler_ref.ternary_read on the same stream"),
    "he_debug_sampler_ternary_words": Row("he_debug_sampler_ternary_words", {"pol": (OUT, Q)}, "sampling.TernarySampler(..., _words=w).Read(pol)",
                                          set(), oracle="tests/sampler_ref.ternary_read(words=w) on the same stream"),
}
