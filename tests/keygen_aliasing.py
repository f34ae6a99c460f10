"""Operand identity at the entry points of include/hering_keygen.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  Every output is distinct from every key operand and
from every other output: no pair that involves an output may be one handle.  An evaluation key and a polynomial are handles of
different kinds and cannot be one object; the pairs a caller can actually form are PAIRS below."""
from tests.aliasing_table import IN, OUT, ACC, P, Q, Row

ORACLE = "tests/keygen_ref on the same stream"
ROWS = {
    "he_keygen_ternary_sparse_read": Row("he_keygen_ternary_sparse_read", {"pol": (OUT, Q)}, "SparseTernarySampler.Read(pol)", set(), oracle=ORACLE),
    "he_keygen_secret_key": Row("he_keygen_secret_key", {"skQ": (OUT, Q), "skP": (OUT, P)}, "KeyGenerator.GenSecretKey(sk)", set(), oracle=ORACLE),
    "he_keygen_secret_key_hw": Row("he_keygen_secret_key_hw", {"skQ": (OUT, Q), "skP": (OUT, P)}, "KeyGenerator.GenSecretKeyWithHammingWeight(hw, sk)",
                                   set(), oracle=ORACLE),
    "he_gadget_add_poly": Row("he_gadget_add_poly", {"pt": (IN, Q), "evk0": (ACC, Q), "evk1": (ACC, Q)},
                              "AddPolyTimesGadgetVectorToGadgetCiphertext(pt, cts)", set(), oracle=ORACLE),
    "he_keygen_evaluation_key": Row("he_keygen_evaluation_key", {"skInQ": (IN, Q), "skOutQ": (IN, Q), "skOutP": (IN, P), "evk": (OUT, Q)},
                                    "KeyGenerator.GenEvaluationKey(skIn, skOut, evk)", set(), oracle=ORACLE),
    "he_keygen_evaluation_key_sk": Row("he_keygen_evaluation_key_sk", {"skInQ": (IN, Q), "skOutQ": (IN, Q), "evk": (OUT, Q)},
                                       "KeyGenerator.GenEvaluationKey(skInput, skOutput, evk)", set(), oracle=ORACLE),
    "he_keygen_relinearization_key": Row("he_keygen_relinearization_key", {"skQ": (IN, Q), "skP": (IN, P), "rlk": (OUT, Q)},
                                         "KeyGenerator.GenRelinearizationKey(sk, rlk)", set(), oracle=ORACLE),
    "he_keygen_galois_key": Row("he_keygen_galois_key", {"skQ": (IN, Q), "skP": (IN, P), "gk": (OUT, Q)}, "KeyGenerator.GenGaloisKey(galEl, sk, gk)",
                                set(), oracle=ORACLE),
    "he_keygen_galois_keys": Row("he_keygen_galois_keys", {"skQ": (IN, Q), "skP": (IN, P), "gks": (OUT, Q)}, "KeyGenerator.GenGaloisKeys(galEls, sk, gks)",
                                 set(), oracle=ORACLE, arrays=("gks",)),
}

# the pairs of one handle a caller can form with an output in them: (entry, parameter a, parameter b); ("gks", "gks"): two entries of
# the array
PAIRS = [("he_keygen_secret_key", "skQ", "skP"), ("he_keygen_secret_key_hw", "skQ", "skP"), ("he_gadget_add_poly", "evk0", "evk1"),
         ("he_keygen_galois_keys", "gks", "gks")]
