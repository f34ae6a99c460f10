"""Operand identity at the entry points of include/hering_encryptor.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  Every output is distinct from every other output, from
the plaintext and from the key polynomials: no pair that involves an output may be one handle.  `key` stands for the polynomials
bound with he_encryptor_set_key / he_decryptor_create, which are operands of the call though not parameters of it."""
from tests.aliasing_table import IN, OUT, P, Q, Row

ORACLE = "tests/encryptor_ref on the same stream"
ROWS = {
    "he_encrypt_zero": Row("he_encrypt_zero", {"c0": (OUT, Q), "c1": (OUT, Q), "key": (IN, Q)}, "Encryptor.EncryptZero(Element)", set(), oracle=ORACLE),
    "he_encrypt_zero_qp": Row("he_encrypt_zero_qp", {"c0Q": (OUT, Q), "c0P": (OUT, P), "c1Q": (OUT, Q), "c1P": (OUT, P), "key": (IN, Q)},
                              "Encryptor.EncryptZero(ElementQP)", set(), oracle=ORACLE),
    "he_add_pt_to_ct": Row("he_add_pt_to_ct", {"pt": (IN, Q), "c0": (OUT, Q)}, "Encryptor.addPtToCt(level, pt, ct)", set(), oracle=ORACLE),
    "he_encrypt": Row("he_encrypt", {"pt": (IN, Q), "c0": (OUT, Q), "c1": (OUT, Q), "key": (IN, Q)}, "Encryptor.Encrypt(pt, ct)", set(), oracle=ORACLE),
    "he_decryptor_decrypt": Row("he_decryptor_decrypt", {"ct": (IN, Q), "pt": (OUT, Q), "key": (IN, Q)}, "Decryptor.Decrypt(ct, pt)", set(),
                                oracle="tests/encryptor_ref.decrypt", arrays=("ct",)),
}


def refused_pairs(row: Row):
    """every pair of the row's operands that must be refused when it is one handle"""
    ps = list(row.params)
    return [(a, b) for i, a in enumerate(ps) for b in ps[i + 1:] if row.verdict(a, b) == "reject"]
