"""Launch census of the key-switch routes: every case runs ONE entry point on seeded words between Context.prof_begin() and
prof_end_bytes() and is held against tests/golden/keyswitch_routes.json:

  (a) the launch profile {kernel name: [launches, algorithmic bytes]} (times left out),
  (b) the SHA-256 of the downloaded words of the polynomials the call writes (one digest over all of them, in operand order),
  (c) the status, for the refused shapes.

The arithmetic is exact and the bytes are computed from shapes, so the file does not depend on the machine.  It was recorded
(`python tests/test_gpu_keyswitch_routes.py --record`) BEFORE the routes moved into csrc/ks_route.h, so it holds the launch
sequence, the limb sets behind every launch and every output word to what the library did then.  The run-time switches are read
once per process: the recorder starts one child per environment (the default one and the four pairs of
tests/test_gpu_fallback_sequences.py, which re-runs this file under each of them), and the file is keyed by the HERING_NO_* names
in effect; an environment's section holds, per case, only the fields that differ from the default section's.

Shapes are the smallest at which a route differs: B = 2, 3-6 Q limbs, 1-2 special primes at logN = 11
(no epilogue, prologue, scatter or giant tail), 12, 13, a conjugate-invariant ring at 12, and B = 1 at logN = 16 (8192-rows) and
at logN = 17 with alpha = 6 (no fused extension)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lattigo_amd as la  # noqa: E402
from lattigo_amd._lib import load  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "keyswitch_routes.json")
# the environments of the recorder: the default one and the pairs of tests/test_gpu_fallback_sequences.py
ENVIRONMENTS = [(), ("HERING_NO_AUTO_SCATTER", "HERING_NO_TENSOR_EPILOGUE"), ("HERING_NO_MAC_EPILOGUE", "HERING_NO_PROD_PROLOGUE"),
                ("HERING_NO_FAST_MODUP", "HERING_NO_LEAN_INV_ROWS"), ("HERING_NO_GIANT_FUSION", "HERING_DRIVER_NO_GIANT")]


def env_key(environ=os.environ):
    names = sorted(k for k, v in environ.items() if k.startswith("HERING_NO_") and v not in ("", "0"))
    return "+".join(names) or "default"


# ring configurations: bit sizes of Q and P (limbs on both sides of 2^47 unless said otherwise)
CFGS = {
    "epi12": dict(logN=12, logq=[55, 45, 58, 45], logp=[61, 60]),        # no special prime below 2^47: the MAC epilogue
    "mix12": dict(logN=12, logq=[55, 45, 58, 45], logp=[61, 46]),        # a special prime below 2^47
    "int12": dict(logN=12, logq=[55, 58, 56, 57], logp=[61, 60]),        # nothing below 2^47: keys without a double-precision copy
    "one12": dict(logN=12, logq=[55, 45, 58], logp=[61]),                # one special prime: base-2 keys with P, RGSW windows
    "nop12": dict(logN=12, logq=[55, 45, 58], logp=[]),                  # no special primes: base-2 keys without P
    "std13": dict(logN=13, logq=[55, 45, 58, 45, 50], logp=[61]),        # a = 1
    "std11": dict(logN=11, logq=[55, 45, 58, 45], logp=[61, 46]),        # plans ok, no epilogue / prologue / scatter / giant tail
    "ci12": dict(logN=12, logq=[55, 45, 58, 45], logp=[61, 60], ci=True),
    "big16": dict(logN=16, logq=[55, 45, 58, 45], logp=[61, 60], B=1),   # 8192-rows
    "big17": dict(logN=17, logq=[55, 45, 58, 45, 56, 46], logp=[61, 60, 59, 58, 57, 56], B=1),  # alpha = 6: nsrc > 5
}
PW2 = 20


class Cfg:
    """rings, evaluator and keys of random words for one configuration; every word is drawn from a generator seeded by name"""

    def __init__(self, ctx, name, logN, logq, logp, ci=False, B=2):
        from oracle import oracle as O
        self.ctx, self.name, self.logN, self.N, self.ci, self.B = ctx, name, logN, 1 << logN, ci, B
        self.q, self.p = O.GenModuli(logN + 2, logq, logp)  # = 1 mod 4N: both ring types, and the half-degree ring
        self.nq, self.np_ = len(self.q), len(self.p)
        self.gQ = la.Ring(ctx, self.N, self.q, conjugate_invariant=ci)
        self.gP = la.Ring(ctx, self.N, self.p, conjugate_invariant=ci) if self.p else None
        self.ev = la.Evaluator(self.gQ, self.gP)
        self.bound = min(self.q + self.p)
        self.gal = pow(5, 3, (4 if ci else 2) * self.N)
        self._keys, self._decs, self._small = {}, {}, None

    def rng(self, tag):
        seed = int.from_bytes(hashlib.sha256(f"{self.name}/{tag}".encode()).digest()[:8], "little")
        return np.random.Generator(np.random.PCG64(seed))

    def words(self, rng, shape):
        return rng.integers(0, self.bound, size=shape, dtype=np.uint64)

    def key(self, kind="rns", idx=0):
        """rns: beta = ceil(nq / np) digits with P; b2: bit windows of PW2 bits, with the evaluator's P (one prime or none)"""
        if (kind, idx) not in self._keys:
            rng = self.rng(f"key/{kind}/{idx}")
            if kind == "rns":
                beta = (self.nq + self.np_ - 1) // self.np_
                kq, kp = self.words(rng, (beta, 2, self.nq, self.N)), self.words(rng, (beta, 2, self.np_, self.N))
                k = self.ev.NewEvaluationKey(kq, kp)
            else:
                nj = [(int(m).bit_length() + PW2 - 1) // PW2 for m in self.q]
                kq = self.words(rng, (sum(nj), 2, self.nq, self.N))
                kp = self.words(rng, (sum(nj), 2, self.np_, self.N)) if self.np_ else None
                k = self.ev.NewEvaluationKey(kq, kp, PW2, nj)
            self._keys[(kind, idx)] = k
        return self._keys[(kind, idx)]

    def dec(self, lq, filled=True):
        """a hoisting buffer of a seeded polynomial at (lq, levelP); filled = False: never filled"""
        if (lq, filled) not in self._decs:
            d = la.rlwe.Decomposition(self.ev, self.B)
            if filled:
                c2 = la.Poly(self.gQ, self.nq, self.B).upload(self.words(self.rng(f"dec/{lq}"), (self.B, self.nq, self.N)))
                self.ev.DecomposeNTT(lq, self.np_ - 1, self.np_, c2, True, d)
            self._decs[(lq, filled)] = d
        return self._decs[(lq, filled)]

    def small_ring(self):
        if self._small is None:
            self._small = la.Ring(self.ctx, self.N // 2, self.q)
        return self._small


class Ops:
    """the operands of one run of a case: seeded inputs, zeroed outputs; `written` collects what the call writes"""

    def __init__(self, c, case_id, B=None):
        self.c, self.B, self.r, self.written, self.inputs = c, c.B if B is None else B, c.rng("case/" + case_id), [], []

    def _in(self, poly):  # (held until the call has run: a handle dies with its Poly)
        self.inputs.append(poly)
        return poly

    def q(self, ring=None):
        ring = ring or self.c.gQ
        return self._in(la.Poly(ring, self.c.nq, self.B).upload(self.c.words(self.r, (self.B, self.c.nq, ring.N))))

    def p(self):
        return self._in(la.Poly(self.c.gP, self.c.np_, self.B).upload(self.c.words(self.r, (self.B, self.c.np_, self.c.N))))

    def out(self, *polys):
        self.written += [x for x in polys if x is not None and all(x is not w for w in self.written)]
        return polys

    def oq(self, ring=None, acc=False):
        ring = ring or self.c.gQ
        return self.out(self.q(ring) if acc else la.Poly(ring, self.c.nq, self.B))[0]

    def op(self, acc=False):
        if self.c.gP is None:
            return None
        return self.out(self.p() if acc else la.Poly(self.c.gP, self.c.np_, self.B))[0]


def _h(p):
    return p.h if p is not None else 0


# ---- the entry points; every function returns the status of the ONE profiled call
def gadget_product(c, o, L, kind="rns", lq=None, alias=False):
    cx = o.q()
    o0 = cx if alias else o.oq()
    o.out(o0)
    return L.he_gadget_product(c.ev.h, c.nq - 1 if lq is None else lq, cx.h, c.key(kind).h, o0.h, o.oq().h)


def gp_lazy(c, o, L, kind="rns", lq=None):
    outs = [o.oq(), o.op(), o.oq(), o.op()]
    return L.he_gadget_product_lazy(c.ev.h, c.nq - 1 if lq is None else lq, o.q().h, c.key(kind).h, *[_h(x) for x in outs])


def gp_hoisted(c, o, L, kind="rns", lazy=False, filled=True, other=None):
    lq = c.nq - 1
    d = (other or c).dec(lq, filled)
    if lazy:
        return L.he_gadget_product_hoisted_lazy(c.ev.h, lq, d.h, c.key(kind).h, o.oq().h, o.op().h, o.oq().h, o.op().h)
    return L.he_gadget_product_hoisted(c.ev.h, lq, d.h, c.key(kind).h, o.oq().h, o.oq().h)


def relinearize(c, o, L, kind="rns", form="plain"):
    i0, i1, i2 = o.q(), o.q(), o.q()
    o0, o1 = {"plain": (None, None), "inplace": (i0, i1), "crossed": (i1, i0)}[form]
    o0, o1 = o0 or o.oq(), o1 or o.oq()
    o.out(o0, o1)
    return L.he_relinearize(c.ev.h, c.nq - 1, i0.h, i1.h, i2.h, c.key(kind).h, o0.h, o1.h)


def automorphism(c, o, L, kind="rns", hoisted=False, alias=False, lq=None):
    lq = c.nq - 1 if lq is None else lq
    i0 = o.q()
    i1 = None if hoisted else o.q()
    o0 = i0 if alias else o.oq()
    o1 = (i1 if alias and i1 is not None else o.oq())
    o.out(o0, o1)
    if hoisted:
        return L.he_automorphism_hoisted(c.ev.h, lq, i0.h, c.dec(lq).h, c.gal, c.key(kind).h, o0.h, o1.h)
    return L.he_automorphism_ct(c.ev.h, lq, i0.h, i1.h, c.gal, c.key(kind).h, o0.h, o1.h)


def auto_hoisted_lazy(c, o, L, alias=False):
    lq = c.nq - 1
    i0 = o.q()
    c0Q = i0 if alias else o.oq()
    o.out(c0Q)
    return L.he_automorphism_hoisted_lazy(c.ev.h, lq, i0.h, c.dec(lq).h, c.gal, c.key().h, c0Q.h, o.op().h, o.oq().h, o.op().h)


def giant_step(c, o, L, kind="rns", acc=0):
    cx, aq, ap = o.q(), o.q(), (o.p() if c.gP is not None else None)
    outs = [o.oq(acc=bool(acc)), o.op(acc=bool(acc)), o.oq(acc=bool(acc)), o.op(acc=bool(acc))]
    return L.he_lintrans_giant_step(c.ev.h, c.nq - 1, cx.h, c.key(kind).h, c.gal, aq.h, _h(ap), *[_h(x) for x in outs], acc)


def mul_relin(c, o, L, kind="rns", bgv=False, alias=False, lq=None):
    lq = c.nq - 1 if lq is None else lq
    a0, a1 = o.q(), o.q()
    b0, b1 = (a0, a1) if alias else (o.q(), o.q())
    o0, o1 = (a0, a1) if alias else (o.oq(), o.oq())
    o.out(o0, o1)
    if bgv:
        return L.he_bgv_mul_relin(c.ev.h, lq, 65537, a0.h, a1.h, b0.h, b1.h, c.key(kind).h, o0.h, o1.h, 0)
    return L.he_ckks_mul_relin(c.ev.h, lq, a0.h, a1.h, b0.h, b1.h, c.key(kind).h, o0.h, o1.h, 0)


def apply_evk(c, o, L, form="same"):
    rin = c.small_ring() if form == "up" else c.gQ
    rout = c.small_ring() if form == "down" else c.gQ
    i0, i1 = o.q(rin), o.q(rin)
    return L.he_apply_evaluation_key(c.ev.h, c.nq - 1, i0.h, i1.h, c.key().h, o.oq(rout).h, o.oq(rout).h)


def ringpack_split(c, o, L):
    s = c.small_ring()
    return L.he_ringpack_split(c.ev.h, c.nq - 1, o.q().h, o.q().h, c.key().h, o.oq(s).h, o.oq(s).h, o.oq(s).h, o.oq(s).h)


def ringpack_merge(c, o, L):
    s = c.small_ring()
    return L.he_ringpack_merge(c.ev.h, c.nq - 1, o.q(s).h, o.q(s).h, o.q(s).h, o.q(s).h, c.key().h, o.oq().h, o.oq().h)


def rgsw(c, o, L, kind="rns"):
    return L.he_rgsw_external_product(c.ev.h, o.q().h, o.q().h, c.key(kind, 0).h, c.key(kind, 1).h, o.oq().h, o.oq().h)


def moddown(c, o, L, lq=None):
    lq = c.nq - 1 if lq is None else lq
    return L.he_moddown(c.ev.h, lq, c.np_ - 1, o.q().h, _h(o.p() if c.gP else None), o.q().h, _h(o.p() if c.gP else None),
                        o.oq().h, o.oq().h)


def eval_moddown(c, o, L):
    return L.he_eval_moddown_qp_to_q_ntt(c.ev.h, c.nq - 1, c.np_ - 1, o.q().h, o.p().h, o.oq().h)


def _case(cid, cfg, fn, B=None, **kw):
    return (cid, cfg, fn, B, kw)


def _cases():
    out = []
    # the route with every fusion: RNS digits, fused extension, MAC epilogue -- every entry point and aliasing pattern
    for cfg in ("epi12",):
        out += [_case(f"{cfg}-gadget_product", cfg, gadget_product), _case(f"{cfg}-gadget_product-out=cx", cfg, gadget_product, alias=True),
                _case(f"{cfg}-gadget_product-below_top", cfg, gadget_product, lq=2),
                _case(f"{cfg}-gp_lazy", cfg, gp_lazy), _case(f"{cfg}-gp_hoisted", cfg, gp_hoisted),
                _case(f"{cfg}-gp_hoisted_lazy", cfg, gp_hoisted, lazy=True)]
        out += [_case(f"{cfg}-relinearize-{f}", cfg, relinearize, form=f) for f in ("plain", "inplace", "crossed")]
        out += [_case(f"{cfg}-automorphism_ct", cfg, automorphism), _case(f"{cfg}-automorphism_ct-out=in", cfg, automorphism, alias=True),
                _case(f"{cfg}-automorphism_ct-below_top", cfg, automorphism, lq=2),
                _case(f"{cfg}-automorphism_hoisted", cfg, automorphism, hoisted=True),
                _case(f"{cfg}-automorphism_hoisted-out=in", cfg, automorphism, hoisted=True, alias=True),
                _case(f"{cfg}-automorphism_hoisted_lazy", cfg, auto_hoisted_lazy),
                _case(f"{cfg}-automorphism_hoisted_lazy-c0Q=in0", cfg, auto_hoisted_lazy, alias=True),
                _case(f"{cfg}-giant_step-acc0", cfg, giant_step, acc=0), _case(f"{cfg}-giant_step-acc1", cfg, giant_step, acc=1),
                _case(f"{cfg}-ckks_mul_relin", cfg, mul_relin), _case(f"{cfg}-ckks_mul_relin-res_res_res", cfg, mul_relin, alias=True),
                _case(f"{cfg}-bgv_mul_relin", cfg, mul_relin, bgv=True), _case(f"{cfg}-bgv_mul_relin-res_res_res", cfg, mul_relin, bgv=True, alias=True),
                _case(f"{cfg}-ckks_mul_relin-below_top", cfg, mul_relin, lq=2)]
        out += [_case(f"{cfg}-apply_evaluation_key-{f}", cfg, apply_evk, form=f) for f in ("same", "down", "up")]
        out += [_case(f"{cfg}-ringpack_split", cfg, ringpack_split), _case(f"{cfg}-ringpack_merge", cfg, ringpack_merge),
                _case(f"{cfg}-rgsw-multiple_p", cfg, rgsw), _case(f"{cfg}-moddown", cfg, moddown),
                # he_eval_moddown_qp_to_q_ntt: below and at one workgroup per CU of the fused extension (B = 7, 8 at 4096-rows)
                _case(f"{cfg}-eval_moddown-B7", cfg, eval_moddown, B=7), _case(f"{cfg}-eval_moddown-B8", cfg, eval_moddown, B=8)]
    # the other selections of facts: one case per (route, entry point)
    for cfg in ("mix12", "int12", "std13", "std11", "ci12"):
        out += [_case(f"{cfg}-gadget_product", cfg, gadget_product), _case(f"{cfg}-gp_lazy", cfg, gp_lazy),
                _case(f"{cfg}-automorphism_ct", cfg, automorphism), _case(f"{cfg}-giant_step-acc1", cfg, giant_step, acc=1),
                _case(f"{cfg}-ckks_mul_relin", cfg, mul_relin), _case(f"{cfg}-relinearize-plain", cfg, relinearize)]
    out += [_case("mix12-bgv_mul_relin-res_res_res", "mix12", mul_relin, bgv=True, alias=True),
            _case("mix12-automorphism_hoisted", "mix12", automorphism, hoisted=True),
            _case("mix12-gadget_product-out=cx", "mix12", gadget_product, alias=True),
            _case("int12-bgv_mul_relin", "int12", mul_relin, bgv=True), _case("int12-giant_step-acc0", "int12", giant_step, acc=0),
            _case("std13-automorphism_hoisted_lazy", "std13", auto_hoisted_lazy), _case("std13-rgsw-windows_pw2_0", "std13", rgsw)]
    for cfg in ("std11", "ci12"):
        out += [_case(f"{cfg}-gp_hoisted", cfg, gp_hoisted), _case(f"{cfg}-automorphism_hoisted", cfg, automorphism, hoisted=True),
                _case(f"{cfg}-automorphism_hoisted_lazy", cfg, auto_hoisted_lazy), _case(f"{cfg}-moddown", cfg, moddown),
                _case(f"{cfg}-eval_moddown-B8", cfg, eval_moddown, B=8), _case(f"{cfg}-apply_evaluation_key-same", cfg, apply_evk)]
    # base-2 keys with and without a special prime; RGSW on the generic route with bit windows
    for cfg in ("one12", "nop12"):
        out += [_case(f"{cfg}-b2-gadget_product", cfg, gadget_product, kind="b2"), _case(f"{cfg}-b2-gp_lazy", cfg, gp_lazy, kind="b2"),
                _case(f"{cfg}-b2-relinearize-inplace", cfg, relinearize, kind="b2", form="inplace"),
                _case(f"{cfg}-b2-automorphism_ct", cfg, automorphism, kind="b2"),
                _case(f"{cfg}-b2-ckks_mul_relin", cfg, mul_relin, kind="b2"), _case(f"{cfg}-b2-rgsw-windows", cfg, rgsw, kind="b2"),
                _case(f"{cfg}-b2-giant_step", cfg, giant_step, kind="b2", acc=0)]  # nop12: refused (no special primes)
    out += [_case("one12-gadget_product", "one12", gadget_product), _case("one12-rgsw-windows_pw2_0", "one12", rgsw),
            _case("nop12-moddown", "nop12", moddown),
            # refused shapes
            _case("one12-b2-gp_hoisted-refused", "one12", gp_hoisted, kind="b2"),
            _case("one12-b2-gp_hoisted_lazy-refused", "one12", gp_hoisted, kind="b2", lazy=True),
            _case("one12-b2-automorphism_hoisted-refused", "one12", automorphism, kind="b2", hoisted=True),
            _case("epi12-gp_hoisted-never_filled", "epi12", gp_hoisted, filled=False)]
    # the two large rings
    out += [_case("big16-gadget_product", "big16", gadget_product), _case("big16-bgv_mul_relin", "big16", mul_relin, bgv=True),
            _case("big16-automorphism_ct", "big16", automorphism), _case("big17-gadget_product", "big17", gadget_product)]
    return out


CASES = _cases()
assert len({c[0] for c in CASES}) == len(CASES)


class Cfgs:
    """the configurations made so far on one context; close() releases every device object while the interpreter is whole (a
    context that survives into interpreter shutdown is never destroyed: its dispatcher thread then outlives the library)"""

    def __init__(self):
        self.ctx, self.made = la.Context(0), {}

    def __call__(self, name):
        if name not in self.made:
            self.made[name] = Cfg(self.ctx, name, **CFGS[name])
        return self.made[name]

    def close(self):
        self.ctx.sync()
        self.made.clear()
        self.ctx.close()


def run_case(cfgs, case):
    """{status, profile, sha256 per written polynomial} of one case; the call runs once unprofiled first, so that what the library
    caches on first use (plans, index tables) is outside the profile whichever cases ran before"""
    cid, cfg, fn, B, kw = case
    c, L = cfgs(cfg), load()
    for profiled in (False, True):
        o = Ops(c, cid, B)
        if profiled:
            c.ctx.sync()
            c.ctx.prof_begin()
        try:
            rc = fn(c, o, L, **kw)
        finally:
            if profiled:
                prof = c.ctx.prof_end_bytes()
        c.ctx.sync()
    rec = {"status": int(rc), "profile": {k: [v[0], v[2]] for k, v in sorted(prof.items())},
           "sha256": hashlib.sha256(b"".join(p.download().tobytes() for p in o.written)).hexdigest()}
    if rc != 0:
        rec["error"] = load().he_last_error().decode().split(":", 1)[-1].strip()
    return rec


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden():
    return _golden()


@pytest.fixture(scope="module")
def cfgs():
    c = Cfgs()
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_route_is_as_recorded(golden, cfgs, case):
    key = env_key()
    assert key in golden, f"no recorded section for the switches {key}"
    assert case[0] in golden["default"], f"{case[0]}: not recorded"
    want = dict(golden["default"][case[0]], **golden[key].get(case[0], {}))
    got = run_case(cfgs, case)
    print(case[0], key, json.dumps(got["profile"]))
    assert got["status"] == want["status"], (got, want)
    assert got.get("error") == want.get("error")
    assert got["profile"] == want["profile"], "launch profile differs from the recorded one"
    assert got["sha256"] == want["sha256"], "output words differ from the recorded ones"


def test_every_recorded_case_still_exists(golden):
    assert set(golden["default"]) == {c[0] for c in CASES}
    assert set(golden) == {env_key({n: "1" for n in names}) for names in ENVIRONMENTS}


# ---- the recorder: one fresh child per environment, one after the other, each under its own time limit
def _record_child(path):
    cfgs = Cfgs()
    try:
        recs = {c[0]: run_case(cfgs, c) for c in CASES}
    finally:
        cfgs.close()
    with open(path, "w") as f:
        json.dump(recs, f)


def _record():
    out = {}
    for names in ENVIRONMENTS:
        env = dict(os.environ)
        for n in list(env):
            if n.startswith("HERING_NO_"):
                del env[n]
        env.update({n: "1" for n in names})
        key = env_key(env)
        tmp = GOLDEN + "." + key + ".tmp"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--record-child", tmp], env=env, cwd=ROOT, timeout=300)
        if r.returncode != 0:
            sys.exit(f"recording under {key} failed with status {r.returncode}: stopping")
        with open(tmp) as f:
            recs = json.load(f)
        os.remove(tmp)
        if key != "default":  # only the fields that differ ("error": only with a status, which no switch changes)
            recs = {k: {f: x for f, x in v.items() if x != out["default"][k].get(f)} for k, v in recs.items()}
            assert all("error" in v or "error" not in out["default"][k] for k, v in recs.items() if "status" in v)
            recs = {k: v for k, v in recs.items() if v}
        out[key] = recs
        print(f"{key}: {len(out[key])} cases kept", flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record-child":
        _record_child(sys.argv[2])
    elif sys.argv[1:] == ["--record"]:
        _record()
    else:
        sys.exit("usage: python tests/test_gpu_keyswitch_routes.py --record")
