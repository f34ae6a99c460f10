"""Operand identity at the entry points of include/hering_multiparty.h, as rows of tests/aliasing_table.Row, in the manner of
tests/keygen_aliasing.py.  A key-shaped operand and a polynomial are handles of different kinds and cannot be one object; among the
key-shaped operands an entry writes one component and reads the other, so the pairs below MAY be one handle, with the same words
as with distinct handles: the rows' `allowed` sets, and ALLOWED, which lists those pairs (entry, parameter a, parameter b) and must agree
with the rows' verdicts.  Polynomial operands that are only read may always be one handle; REFUSED lists the pairs with a written
operand that the GPU test tries."""
from tests.aliasing_table import IN, OUT, ACC, P, Q, Row

ORACLE = "tests/multiparty_ref on the same streams"
ROWS = {
    "he_mp_crp_gadget": Row("he_mp_crp_gadget", {"evk": (ACC, Q)}, "EvaluationKeyGenProtocol.SampleCRP(crs)", set(), oracle=ORACLE),
    "he_mp_evk_gen_share": Row("he_mp_evk_gen_share", {"skInQ": (IN, Q), "skOutQ": (IN, Q), "skOutP": (IN, P), "crp": (IN, Q), "share": (ACC, Q)},
                               "EvaluationKeyGenProtocol.GenShare(skIn, skOut, crp, shareOut)", {("share", "crp")}, oracle=ORACLE),
    "he_mp_galois_gen_share": Row("he_mp_galois_gen_share", {"skQ": (IN, Q), "skP": (IN, P), "crp": (IN, Q), "share": (ACC, Q)},
                                  "GaloisKeyGenProtocol.GenShare(sk, galEl, crp, shareOut)", {("share", "crp")}, oracle=ORACLE),
    "he_mp_gadget_aggregate": Row("he_mp_gadget_aggregate", {"a": (IN, Q), "b": (IN, Q), "out": (ACC, Q)},
                                  "EvaluationKeyGenProtocol.AggregateShares(share1, share2, share3)", {("out", "a"), ("out", "b")}, oracle=ORACLE),
    "he_mp_rkg_round_one": Row("he_mp_rkg_round_one", {"skQ": (IN, Q), "skP": (IN, P), "crp": (IN, Q), "ephQ": (OUT, Q), "ephP": (OUT, P), "share1": (OUT, Q)},
                               "RelinearizationKeyGenProtocol.GenShareRoundOne(sk, crp, ephSkOut, shareOut)", set(), oracle=ORACLE),
    "he_mp_rkg_round_two": Row("he_mp_rkg_round_two", {"ephQ": (IN, Q), "ephP": (IN, P), "skQ": (IN, Q), "skP": (IN, P), "round1": (IN, Q), "share2": (ACC, Q)},
                               "RelinearizationKeyGenProtocol.GenShareRoundTwo(ephSk, sk, round1, shareOut)", set(), oracle=ORACLE),
    "he_mp_rlk_finalize": Row("he_mp_rlk_finalize", {"round1": (IN, Q), "round2": (IN, Q), "rlk": (OUT, Q)},
                              "RelinearizationKeyGenProtocol.GenRelinearizationKey(round1, round2, evalKeyOut)", {("rlk", "round1"), ("rlk", "round2")},
                              oracle=ORACLE),
    "he_mp_pk_gen_share": Row("he_mp_pk_gen_share", {"skQ": (IN, Q), "skP": (IN, P), "crpQ": (IN, Q), "crpP": (IN, P), "shareQ": (OUT, Q), "shareP": (OUT, P)},
                              "PublicKeyGenProtocol.GenShare(sk, crp, shareOut)", set(), oracle=ORACLE),
    "he_mp_cks_gen_share": Row("he_mp_cks_gen_share", {"skInQ": (IN, Q), "skOutQ": (IN, Q), "c1": (IN, Q), "share": (OUT, Q)},
                               "KeySwitchProtocol.GenShare(skInput, skOutput, ct, shareOut)", set(), oracle=ORACLE),
    "he_mp_pcks_gen_share": Row("he_mp_pcks_gen_share", {"skQ": (IN, Q), "c1": (IN, Q), "share0": (OUT, Q), "share1": (OUT, Q)},
                                "PublicKeySwitchProtocol.GenShare(sk, pk, ct, shareOut)", set(), oracle=ORACLE),
    "he_mp_evk_finalize": Row("he_mp_evk_finalize", {"share": (IN, Q), "crp": (IN, Q), "evk": (ACC, Q)},
                              "EvaluationKeyGenProtocol.GenEvaluationKey(share, crp, evk)", {("evk", "share"), ("evk", "crp")}, oracle=ORACLE),
}

# the key-shaped parameters of each entry (every other parameter is a polynomial)
KEYS = {"he_mp_crp_gadget": ("evk",), "he_mp_evk_gen_share": ("crp", "share"), "he_mp_galois_gen_share": ("crp", "share"),
        "he_mp_gadget_aggregate": ("a", "b", "out"), "he_mp_evk_finalize": ("share", "crp", "evk"), "he_mp_rkg_round_one": ("crp", "share1"),
        "he_mp_rkg_round_two": ("round1", "share2"), "he_mp_rlk_finalize": ("round1", "round2", "rlk"), "he_mp_pk_gen_share": (),
        "he_mp_cks_gen_share": (), "he_mp_pcks_gen_share": ()}
# the pairs of key-shaped parameters that may be one handle
ALLOWED = [("he_mp_evk_gen_share", "crp", "share"), ("he_mp_galois_gen_share", "crp", "share"),
           ("he_mp_gadget_aggregate", "a", "b"), ("he_mp_gadget_aggregate", "a", "out"), ("he_mp_gadget_aggregate", "b", "out"),
           ("he_mp_evk_finalize", "share", "crp"), ("he_mp_evk_finalize", "share", "evk"), ("he_mp_evk_finalize", "crp", "evk"),
           ("he_mp_rlk_finalize", "round1", "round2"), ("he_mp_rlk_finalize", "round1", "rlk"), ("he_mp_rlk_finalize", "round2", "rlk")]
# the pairs a caller can form that are refused (HE_EINVAL): a written operand with another operand of its kind
REFUSED = [("he_mp_rkg_round_one", "crp", "share1"), ("he_mp_rkg_round_two", "round1", "share2"),
           ("he_mp_rkg_round_one", "skQ", "ephQ"), ("he_mp_rkg_round_one", "skP", "ephP"), ("he_mp_rkg_round_one", "ephQ", "ephP"),
           ("he_mp_pk_gen_share", "skQ", "shareQ"), ("he_mp_pk_gen_share", "crpQ", "shareQ"), ("he_mp_pk_gen_share", "skP", "shareP"),
           ("he_mp_pk_gen_share", "crpP", "shareP"), ("he_mp_pk_gen_share", "shareQ", "shareP"),
           ("he_mp_cks_gen_share", "skInQ", "share"), ("he_mp_cks_gen_share", "skOutQ", "share"), ("he_mp_cks_gen_share", "c1", "share"),
           ("he_mp_pcks_gen_share", "skQ", "share0"), ("he_mp_pcks_gen_share", "c1", "share1"), ("he_mp_pcks_gen_share", "share0", "share1")]
