"""Operand identity at the entry points of include/hering_rgsw_encryptor.h, as rows of tests/aliasing_table.Row, in the manner of
tests/keygen_aliasing.py.  Every output key is distinct from every other output key; the plaintext, the LWE secret and the bound
secret key are polynomials, handles of another kind than a key, and cannot be one object with an output.  The pairs a caller can
actually form are PAIRS below."""
from tests.aliasing_table import IN, OUT, Q, Row

ORACLE = "tests/rgsw_encryptor_ref on the same stream"
ROWS = {
    "he_rgsw_encrypt_zero": Row("he_rgsw_encrypt_zero", {"rgsw0": (OUT, Q), "rgsw1": (OUT, Q)}, "rgsw.Encryptor.EncryptZero(ct)", set(), oracle=ORACLE),
    "he_rgsw_encrypt": Row("he_rgsw_encrypt", {"pt": (IN, Q), "rgsw0": (OUT, Q), "rgsw1": (OUT, Q)}, "rgsw.Encryptor.Encrypt(pt, ct)", set(), oracle=ORACLE),
    "he_rgsw_encrypt_table": Row("he_rgsw_encrypt_table", {"pts": (IN, Q), "rgsw0": (OUT, Q), "rgsw1": (OUT, Q)},
                                 "rgsw.Encryptor.EncryptTable(pts, sel, cts)", set(), oracle=ORACLE, arrays=("rgsw0", "rgsw1")),
    "he_blindrot_gen_evaluation_key": Row("he_blindrot_gen_evaluation_key", {"skLWE": (IN, Q), "rgsw0": (OUT, Q), "rgsw1": (OUT, Q), "gks": (OUT, Q)},
                                          "blindrot.GenEvaluationKeyNew(paramsRLWE, skRLWE, paramsLWE, skLWE)", set(), oracle=ORACLE,
                                          arrays=("rgsw0", "rgsw1", "gks")),
}

# the pairs of one handle a caller can form with an output in them: (entry, parameter a, parameter b); a parameter paired with
# itself: two entries of the array
PAIRS = [("he_rgsw_encrypt_zero", "rgsw0", "rgsw1"), ("he_rgsw_encrypt", "rgsw0", "rgsw1"),
         ("he_rgsw_encrypt_table", "rgsw0", "rgsw1"), ("he_rgsw_encrypt_table", "rgsw0", "rgsw0"), ("he_rgsw_encrypt_table", "rgsw1", "rgsw1"),
         ("he_blindrot_gen_evaluation_key", "rgsw0", "rgsw1"), ("he_blindrot_gen_evaluation_key", "rgsw0", "rgsw0"),
         ("he_blindrot_gen_evaluation_key", "rgsw1", "rgsw1"), ("he_blindrot_gen_evaluation_key", "gks", "gks"),
         ("he_blindrot_gen_evaluation_key", "rgsw0", "gks"), ("he_blindrot_gen_evaluation_key", "rgsw1", "gks")]
