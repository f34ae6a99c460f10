#!/usr/bin/env python3
"""The check of go/hering/*.go that is possible without a Go toolchain: every `C.he_*(...)` call names a function
declared in include/hering.h (or hering_debug.h, hering_ringswitch.h, hering_ringpack.h, hering_rgsw.h, hering_blindrot.h, hering_bridge.h, hering_bfv.h, hering_ckks_encoder.h, hering_bgv_encoder.h, hering_sampler.h, hering_encryptor.h, hering_keygen.h, hering_rgsw_encryptor.h, hering_multiparty.h, hering_lintrans.h, hering_polyeval.h, hering_ckks_evaluator.h), passes as many arguments as the declaration has parameters, and -- round 4 --
every argument has the KIND the parameter wants (int / uint64_t / he_handle / he_handle* / uint64_t* / int*), judged from the
shape of the Go expression (`C.int(..)`, `C.uint64_t(..)`, `x.h`, `&x.h`, `(*C.uint64_t)(unsafe.Pointer(..))`, identifiers whose
declaration in the file names a Handle or a C pointer type); every `C.HE_*` constant exists in the header's enums.  Also
lists which of rlwe.EvaluatorProvider's seven methods and of schemes.Evaluator's methods the Go package defines.  It is not a type
checker: the package has still never met the Go compiler.

    python tools/check_go_abi.py            # exit status 0 when everything matches
"""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_decls():
    src = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("hering.h", "hering_debug.h", "hering_ringswitch.h", "hering_ringpack.h", "hering_rgsw.h", "hering_blindrot.h", "hering_bridge.h", "hering_bfv.h", "hering_ckks_encoder.h", "hering_bgv_encoder.h", "hering_sampler.h", "hering_encryptor.h", "hering_keygen.h", "hering_rgsw_encryptor.h", "hering_multiparty.h", "hering_lintrans.h", "hering_polyeval.h", "hering_ckks_evaluator.h"))
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls, kinds = {}, {}
    for m in re.finditer(r"\b(?:int|const char \*)\s*(he_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        params = m.group(2).strip()
        plist = [] if params in ("", "void") else split_args(params)
        decls[m.group(1)] = len(plist)
        kinds[m.group(1)] = [param_kind(p) for p in plist]
    consts = set(re.findall(r"\b(HE_[A-Z0-9_]+)\b", src))
    return decls, consts, kinds


def param_kind(p):
    """kind of a C parameter declaration"""
    p = " ".join(p.replace("const", " ").split())
    ptr = "*" in p or "[" in p
    if "he_handle" in p:
        return "handle*" if ptr else "handle"
    if "uint64_t" in p:
        return "u64*" if ptr else "u64"
    if "uint8_t" in p:
        return "u8*" if ptr else "u8"
    if re.match(r"^(int|size_t)\b", p) and not ptr:
        return "int"
    if re.match(r"^int\b", p) and ptr:
        return "int*"
    return "other"


def arg_kind(a, src):
    """kind of a Go argument expression, or None when its shape says nothing"""
    a = a.strip()
    if re.match(r"^C\.int\(", a) or re.match(r"^C\.HE_[A-Z0-9_]+$", a) or re.match(r"^C\.size_t\(", a):
        return "int"
    if re.match(r"^C\.uint64_t\(", a):
        return "u64"
    if re.match(r"^\(\*C\.uint64_t\)\(unsafe\.Pointer\(", a):
        return "u64*"
    if re.match(r"^\(\*C\.uint8_t\)\(unsafe\.Pointer\(", a):
        return "u8*"
    if re.match(r"^&[\w.\[\]]+\.h$", a):
        return "handle*"
    if re.match(r"^[\w.\[\]]+\.h$", a) or re.match(r"^h\(\w+\)$", a):
        return "handle"
    m = re.match(r"^&(\w+)\[0\]$", a)
    if m and re.search(r"\b%s\s*:?=\s*make\(\[\]C\.int\b" % m.group(1), src):
        return "int*"
    m = re.match(r"^(\w+)(\[\d+\])?$", a)
    if m:
        name = m.group(1)
        if re.search(r"\bvar\s+%s\s+(\[\d+\])?Handle\b" % name, src) or re.search(r"\b%s\s+(\[\d+\])?Handle\b" % name, src):
            return "handle"
        if re.search(r"\bvar\s+%s\s+\*C\.uint64_t\b" % name, src):
            return "u64*"
    return None


def split_args(s):
    """top-level comma split (parentheses / brackets / braces nest)"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur)
    return out


def go_calls(path):
    src = open(path).read()
    src = re.sub(r"//[^\n]*", "", src)
    for m in re.finditer(r"\bC\.(he_[a-z0-9_]+)\s*\(", src):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        args = split_args(src[m.end():i - 1])
        yield m.group(1), args, src.count("\n", 0, m.start()) + 1, src
    for m in re.finditer(r"\bC\.(HE_[A-Z0-9_]+)\b", src):
        yield m.group(1), None, src.count("\n", 0, m.start()) + 1, src


PROVIDER = ["DecomposeNTT", "CheckAndGetGaloisKey", "GadgetProductLazy", "GadgetProductHoistedLazy", "AutomorphismHoistedLazy",
            "ModDownQPtoQNTT", "AutomorphismIndex"]                                   # core/rlwe/rlwe.go:10-18
# rlwe.Evaluator methods outside both interfaces that the package defines as well
EXTRA = ["ApplyEvaluationKey"]                                                        # core/rlwe/evaluator_evaluationkey.go:36
# rlwe.RingPackingEvaluator (go/hering/ringpack.go)
RINGPACK = ["Split", "Merge"]                                                         # core/rlwe/ring_packing.go:173,376
# rgsw.Evaluator (go/hering/rgsw.go)
RGSW = ["ExternalProduct"]                                                            # core/rgsw/evaluator.go:39
# blindrot.Evaluator and its key sets (go/hering/blindrot.go)
BLINDROT = ["BlindRotateCore", "AutomorphismSelect"]                                  # core/rgsw/blindrot/evaluator.go:135
# ckks.DomainSwitcher (go/hering/bridge.go)
BRIDGE = ["ComplexToReal", "RealToComplex"]                                           # schemes/ckks/bridge.go:57,104
# bgv.Evaluator with ScaleInvariant = true (go/hering/bfv.go)
BFV = ["MulScaleInvariant", "MulScaleInvariantNew", "MulRelinScaleInvariant", "MulRelinScaleInvariantNew"]  # schemes/bgv/evaluator.go:705-895
# ckks.Encoder, double-precision path (go/hering/encoder.go)
ENCODER = ["Encode", "Embed", "Decode", "DecodePublic", "FFT", "IFFT"]                # schemes/ckks/encoder.go:156-820
# bgv.Encoder (go/hering/bgv_encoder.go)
BGV_ENCODER = ["Encode", "Embed", "EmbedScale", "Decode", "EncodeRingT", "DecodeRingT", "RingT2Q", "RingQ2T"]  # schemes/bgv/encoder.go:143-526
# ring.UniformSampler / GaussianSampler / TernarySampler (go/hering/sampler.go)
SAMPLERS = {"UniformSampler": ["Read", "ReadAndAdd", "ReadQP", "ReadAndAddQP", "AtLevel"], "GaussianSampler": ["Read", "ReadAndAdd", "AtLevel"],
            "TernarySampler": ["Read", "ReadAndAdd", "AtLevel"]}                      # ring/sampler_uniform.go, sampler_gaussian.go, sampler_ternary.go
# rlwe.KeyGenerator (go/hering/keygen.go)
KEYGEN = ["GenSecretKey", "GenSecretKeyWithHammingWeight", "GenPublicKey", "GenRelinearizationKey", "GenGaloisKey", "GenGaloisKeys",
          "GenEvaluationKey", "NewEvaluationKey"]                                    # core/rlwe/keygenerator.go:37-285
# lintrans.Evaluator (go/hering/lintrans.go)
LINTRANS = ["EvaluateMany", "Evaluate"]                                               # circuits/common/lintrans/lintrans_evaluator.go:27,122
SCHEMES = ["Add", "AddNew", "Sub", "SubNew", "Mul", "MulNew", "MulRelin", "MulRelinNew", "MulThenAdd", "Relinearize",
           "Rescale", "GetRLWEParameters"]                                            # schemes/schemes.go:14-28


def main():
    decls, consts, kinds = header_decls()
    errors, ncalls, used, nchecked, nargs_total = [], 0, set(), 0, 0
    files = sorted(glob.glob(os.path.join(ROOT, "go", "hering", "*.go")))
    for f in files:
        for name, args, line, gosrc in go_calls(f):
            where = f"{os.path.relpath(f, ROOT)}:{line}"
            if args is None:
                if name not in consts:
                    errors.append(f"{where}: constant {name} is not in the header")
                continue
            ncalls += 1
            used.add(name)
            if name not in decls:
                errors.append(f"{where}: {name} is not declared in include/*.h")
            elif decls[name] != len(args):
                errors.append(f"{where}: {name} called with {len(args)} arguments, declared with {decls[name]}")
            else:
                for i, (a, want) in enumerate(zip(args, kinds[name])):
                    nargs_total += 1
                    got = arg_kind(a, gosrc)
                    if got is None or want == "other":
                        continue
                    nchecked += 1
                    if got != want:
                        errors.append(f"{where}: {name} argument {i + 1} `{a.strip()}` looks like {got}, the header wants {want}")
    for f in files:  # a structural sanity check of each file: brackets balance outside strings, runes and comments
        txt = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(f).read(), flags=re.S)
        txt = re.sub(r'"(?:\\.|[^"\\\n])*"|`[^`]*`|\'(?:\\.|[^\'\\])\'', '""', txt)
        for o, c in ("{}", "()", "[]"):
            if txt.count(o) != txt.count(c):
                errors.append(f"{os.path.relpath(f, ROOT)}: {txt.count(o)} '{o}' against {txt.count(c)} '{c}'")
    src = "".join(open(f).read() for f in files)
    methods = set(re.findall(r"func \(\w+ \*(?:Evaluator|SchemeEvaluator)\) (\w+)\(", src))
    for m in PROVIDER + SCHEMES:
        if m not in methods:
            errors.append(f"go/hering: method {m} (rlwe.EvaluatorProvider / schemes.Evaluator) is not defined")
    for m in EXTRA:
        if m not in methods:
            errors.append(f"go/hering: method {m} (rlwe.Evaluator) is not defined")
    rp_methods = set(re.findall(r"func \(\w+ \*RingPackingEvaluator\) (\w+)\(", src))
    for m in RINGPACK:
        if m not in rp_methods:
            errors.append(f"go/hering: method {m} (rlwe.RingPackingEvaluator) is not defined")
    rgsw_methods = set(re.findall(r"func \(\w+ \*RGSWEvaluator\) (\w+)\(", src))
    for m in RGSW:
        if m not in rgsw_methods:
            errors.append(f"go/hering: method {m} (rgsw.Evaluator) is not defined")
    br_methods = set(re.findall(r"func \(\w+ \*BlindRotationEvaluator\) (\w+)\(", src))
    for m in BLINDROT:
        if m not in br_methods:
            errors.append(f"go/hering: method {m} (blindrot.Evaluator) is not defined")
    ds_methods = set(re.findall(r"func \(\w+ \*DomainSwitcher\) (\w+)\(", src))
    for m in BRIDGE:
        if m not in ds_methods:
            errors.append(f"go/hering: method {m} (ckks.DomainSwitcher) is not defined")
    bfv_methods = set(re.findall(r"func \(\w+ \*ScaleInvariantEvaluator\) (\w+)\(", src))
    for m in BFV:
        if m not in bfv_methods:
            errors.append(f"go/hering: method {m} (bgv.Evaluator, scale-invariant) is not defined")
    enc_methods = set(re.findall(r"func \(\w+ \*Encoder\) (\w+)\(", src))
    for m in ENCODER:
        if m not in enc_methods:
            errors.append(f"go/hering: method {m} (ckks.Encoder) is not defined")
    bgv_enc_methods = set(re.findall(r"func \(\w+ \*BGVEncoder\) (\w+)\(", src))
    for m in BGV_ENCODER:
        if m not in bgv_enc_methods:
            errors.append(f"go/hering: method {m} (bgv.Encoder) is not defined")
    for t, want in SAMPLERS.items():
        have = set(re.findall(r"func \(\w+ \*%s\) (\w+)\(" % t, src))
        for m in want:
            if m not in have:
                errors.append(f"go/hering: method {m} (ring.{t}) is not defined")
    kg_methods = set(re.findall(r"func \(\w+ \*KeyGenerator\) (\w+)\(", src))
    for m in KEYGEN:
        if m not in kg_methods:
            errors.append(f"go/hering: method {m} (rlwe.KeyGenerator) is not defined")
    lt_methods = set(re.findall(r"func \(\w+ \*LinTransEvaluator\) (\w+)\(", src))
    for m in LINTRANS:
        if m not in lt_methods:
            errors.append(f"go/hering: method {m} (lintrans.Evaluator) is not defined")
    print(f"{len(files)} Go files, {ncalls} C.he_* calls to {len(used)} of {len(decls)} declared entry points, {nchecked} of {nargs_total} "
          f"arguments kind-checked; {len(PROVIDER)} EvaluatorProvider + {len(SCHEMES)} schemes.Evaluator methods present; "
          f"rlwe.Evaluator also: {', '.join(m for m in EXTRA if m in methods)}; "
          f"rlwe.RingPackingEvaluator: {', '.join(m for m in RINGPACK if m in rp_methods)}; "
          f"rgsw.Evaluator: {', '.join(m for m in RGSW if m in rgsw_methods)}; "
          f"blindrot.Evaluator: {', '.join(m for m in BLINDROT if m in br_methods)}; "
          f"ckks.DomainSwitcher: {', '.join(m for m in BRIDGE if m in ds_methods)}; "
          f"bgv.Evaluator (scale-invariant): {', '.join(m for m in BFV if m in bfv_methods)}; "
          f"ckks.Encoder: {', '.join(m for m in ENCODER if m in enc_methods)}; "
          f"bgv.Encoder: {', '.join(m for m in BGV_ENCODER if m in bgv_enc_methods)}; "
          f"ring samplers: {', '.join(SAMPLERS)}; "
          f"rlwe.KeyGenerator: {', '.join(m for m in KEYGEN if m in kg_methods)}; "
          f"lintrans.Evaluator: {', '.join(m for m in LINTRANS if m in lt_methods)}"
          if not errors else "\n".join(errors))
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
