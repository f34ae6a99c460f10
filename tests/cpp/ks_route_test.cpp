// ks_route() (lattigo_amd/csrc/ks_route.h) over EVERY combination of KsFacts: the invariants the launch code relies on, and one
// pinned route per row of the table in DESIGN.md section 4.  Plain host C++, no device and no library.
#include <cstdio>
#include <cstdlib>

#include "ks_route.h"

static long g_checked = 0, g_failed = 0;

static void describe(const KsFacts &f) {
    std::fprintf(stderr,
                 "  facts: form %d ring %d pw2 %d keyd %d levelP %d p_class2 %d f64 %d dec_ok %d md_ok %d | supported prod %d scat %d epi %d giant %d | "
                 "alias operand %d addend %d crossed %d | no_mac %d no_prod %d no_tensor %d no_scatter %d no_giant %d\n",
                 (int)f.form, f.ring_type, f.pw2, f.keyd, f.levelP, f.p_class2, f.f64_tables, f.dec_ok, f.md_ok, f.prod_in_supported,
                 f.scatter_supported, f.mac_epilogue_supported, f.mac_giant_supported, f.alias.out_is_operand, f.alias.out_is_addend, f.alias.crossed,
                 f.no_mac_epilogue, f.no_prod_prologue, f.no_tensor_epilogue, f.no_auto_scatter, f.no_giant_fusion);
}
#define CHECK(f, cond)                                                    \
    do {                                                                  \
        g_checked++;                                                      \
        if (!(cond)) {                                                    \
            if (g_failed++ < 20) {                                        \
                std::fprintf(stderr, "FAIL line %d: %s\n", __LINE__, #cond); \
                describe(f);                                              \
            }                                                             \
        }                                                                 \
    } while (0)
#define IMPLIES(f, a, b) CHECK(f, !(a) || (b))

static bool fused_moddown(const KsRoute &r) { return r.moddown == KS_MD_FUSED_ROWS || r.moddown == KS_MD_FUSED_MAC; }
// every fusion a switch can take away, as a number: a switch may only lower it
static bool no_more_fused(const KsRoute &off, const KsRoute &on) {
    return (!off.prod_prologue || on.prod_prologue) && (!off.tensor_epilogue || on.tensor_epilogue) && (!off.giant_fused || on.giant_fused) &&
           (off.moddown != KS_MD_FUSED_MAC || on.moddown == KS_MD_FUSED_MAC) &&
           (off.automorphism == on.automorphism || off.automorphism == KS_AUTO_GATHERS);
}

static void invariants(const KsFacts &f) {
    const KsRoute r = ks_route(f);
    const bool standard = f.ring_type == 0;
    const bool automorphism = f.form == KS_AUTOMORPHISM || f.form == KS_AUTOMORPHISM_HOISTED;
    const bool any_alias = f.alias.out_is_operand || f.alias.out_is_addend || f.alias.crossed;
    // the MAC epilogue
    IMPLIES(f, r.moddown == KS_MD_FUSED_MAC, f.md_ok && f.keyd && !f.p_class2 && r.digits == KS_DIGITS_FUSED && r.mac_f64 && !f.pw2 && standard);
    IMPLIES(f, r.moddown == KS_MD_FUSED_MAC, f.mac_epilogue_supported && !f.no_mac_epilogue);
    // ... never writes the operand: no output is the operand, or the key switch writes the temporaries of the gather form
    IMPLIES(f, r.moddown == KS_MD_FUSED_MAC, !f.alias.out_is_operand || r.automorphism == KS_AUTO_GATHERS);
    IMPLIES(f, r.moddown == KS_MD_FUSED_MAC, !r.acc_q_f64);
    IMPLIES(f, r.acc_q_f64, r.moddown == KS_MD_FUSED_ROWS && r.mac_f64);
    IMPLIES(f, r.mac_f64, f.keyd && r.digits == KS_DIGITS_FUSED);
    IMPLIES(f, r.digits == KS_DIGITS_FUSED, f.dec_ok && standard && !f.pw2 && f.levelP >= 0);
    IMPLIES(f, fused_moddown(r), f.md_ok && standard && f.levelP >= 0);
    IMPLIES(f, f.levelP < 0, r.moddown == KS_MD_NONE);
    // the epilogue scatter
    IMPLIES(f, r.automorphism == KS_AUTO_EPILOGUE_SCATTER, fused_moddown(r) && standard && !any_alias && automorphism && f.scatter_supported);
    // (the giant step accepts no aliasing at all: its entry point passes none)
    IMPLIES(f, r.automorphism == KS_AUTO_KS_SCATTER, standard && (r.giant_fused || (f.form == KS_AUTOMORPHISM_HOISTED_LAZY && !any_alias)));
    IMPLIES(f, r.automorphism != KS_AUTO_NONE, automorphism || f.form == KS_AUTOMORPHISM_HOISTED_LAZY || f.form == KS_GIANT_STEP);
    IMPLIES(f, automorphism || f.form == KS_AUTOMORPHISM_HOISTED_LAZY || f.form == KS_GIANT_STEP, r.automorphism != KS_AUTO_NONE);
    // the tensor terms in the epilogue
    IMPLIES(f, r.tensor_epilogue, fused_moddown(r) && !f.alias.out_is_addend && f.form == KS_MUL_RELIN);
    IMPLIES(f, r.prod_prologue, r.tensor_epilogue && r.digits == KS_DIGITS_FUSED && f.prod_in_supported && f.f64_tables);
    // the fused giant step
    IMPLIES(f, r.giant_fused, r.digits == KS_DIGITS_FUSED && standard && f.form == KS_GIANT_STEP && r.moddown == KS_MD_NONE);
    IMPLIES(f, r.giant_fused, !f.keyd || f.mac_giant_supported);
    // entry tables: every selected stage is table-capable
    IMPLIES(f, r.tables_ok, standard && (r.digits == KS_DIGITS_FUSED || r.digits == KS_DIGITS_GIVEN || f.form == KS_MUL_RELIN));
    IMPLIES(f, r.tables_ok && f.form != KS_HOISTED && f.form != KS_LAZY && f.form != KS_GIANT_STEP, fused_moddown(r));
    // (the forms whose entry points accept an output that is an input; MulRelin's operand is scratch)
    IMPLIES(f, r.tables_ok && (f.form == KS_GADGET_PRODUCT || automorphism), !f.alias.out_is_operand && !f.alias.crossed);
    IMPLIES(f, r.tables_ok && automorphism, !any_alias);
    IMPLIES(f, f.form == KS_AUTOMORPHISM_HOISTED_LAZY, !r.tables_ok);
    // hoisted forms never make digits; a base-2 gadget never takes RNS digits
    IMPLIES(f, f.form == KS_HOISTED || f.form == KS_AUTOMORPHISM_HOISTED || f.form == KS_AUTOMORPHISM_HOISTED_LAZY, r.digits == KS_DIGITS_GIVEN);
    IMPLIES(f, f.pw2 && r.digits != KS_DIGITS_GIVEN, r.digits == KS_DIGITS_WINDOWS);
    // each switch only ever turns fields off, and changes nothing else
    bool KsFacts::*const switches[5] = {&KsFacts::no_mac_epilogue, &KsFacts::no_prod_prologue, &KsFacts::no_tensor_epilogue,
                                        &KsFacts::no_auto_scatter, &KsFacts::no_giant_fusion};
    for (bool KsFacts::*sw : switches) {
        if (f.*sw) continue;
        KsFacts g = f;
        g.*sw = true;
        const KsRoute o = ks_route(g);
        CHECK(g, no_more_fused(o, r));
        CHECK(g, o.digits == r.digits && o.mac_f64 == r.mac_f64 && o.tables_ok == r.tables_ok && fused_moddown(o) == fused_moddown(r));
    }
    KsFacts g = f;
    g.no_mac_epilogue = true;
    CHECK(g, ks_route(g).moddown != KS_MD_FUSED_MAC);
    g = f; g.no_prod_prologue = true;
    CHECK(g, !ks_route(g).prod_prologue);
    g = f; g.no_tensor_epilogue = true;
    CHECK(g, !ks_route(g).tensor_epilogue && !ks_route(g).prod_prologue);
    g = f; g.no_auto_scatter = true;
    CHECK(g, ks_route(g).automorphism == KS_AUTO_NONE || ks_route(g).automorphism == KS_AUTO_GATHERS);
    CHECK(g, !ks_route(g).giant_fused);
    g = f; g.no_giant_fusion = true;
    CHECK(g, !ks_route(g).giant_fused);
}

// ---- one named route per row of DESIGN.md section 4
static KsFacts all_fused(KsForm form) {  // standard ring, RNS key with a double-precision copy, integer special primes, both plans
    KsFacts f;
    f.form = form; f.keyd = true; f.levelP = 1; f.f64_tables = true; f.dec_ok = f.md_ok = true;
    f.prod_in_supported = f.scatter_supported = f.mac_epilogue_supported = f.mac_giant_supported = true;
    return f;
}
static bool same(const KsRoute &a, const KsRoute &b) {
    return a.digits == b.digits && a.mac_f64 == b.mac_f64 && a.prod_prologue == b.prod_prologue && a.moddown == b.moddown &&
           a.acc_q_f64 == b.acc_q_f64 && a.tensor_epilogue == b.tensor_epilogue && a.automorphism == b.automorphism &&
           a.giant_fused == b.giant_fused && a.tables_ok == b.tables_ok;
}
static KsRoute route(KsDigits d, bool mac, bool prologue, KsModDown md, bool acc64, bool tensor, KsAuto au, bool giant, bool tables) {
    KsRoute r;
    r.digits = d; r.mac_f64 = mac; r.prod_prologue = prologue; r.moddown = md; r.acc_q_f64 = acc64; r.tensor_epilogue = tensor;
    r.automorphism = au; r.giant_fused = giant; r.tables_ok = tables;
    return r;
}
#define PIN(name, facts, ...)                                                       \
    do {                                                                            \
        g_checked++;                                                                \
        if (!same(ks_route(facts), route(__VA_ARGS__))) {                           \
            g_failed++;                                                             \
            std::fprintf(stderr, "FAIL pinned route \"%s\"\n", name);               \
            describe(facts);                                                        \
        }                                                                           \
    } while (0)

static void pinned() {
    KsFacts f = all_fused(KS_GADGET_PRODUCT);
    PIN("MAC epilogue", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_NONE, false, true);
    f.alias.out_is_operand = true;
    PIN("output is the operand: rows epilogue over double accumulators", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_ROWS, true, false, KS_AUTO_NONE, false, false);
    f = all_fused(KS_GADGET_PRODUCT); f.p_class2 = true;
    PIN("a special prime below 2^47", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_ROWS, true, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_GADGET_PRODUCT); f.mac_epilogue_supported = false;
    PIN("rows of another size (logN <= 11)", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_ROWS, true, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_GADGET_PRODUCT); f.keyd = false; f.f64_tables = false;
    PIN("no modulus below 2^47", f, KS_DIGITS_FUSED, false, false, KS_MD_FUSED_ROWS, false, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_GADGET_PRODUCT); f.dec_ok = f.md_ok = false;
    PIN("no fused extension (alpha > 5 at logN = 17)", f, KS_DIGITS_UNFUSED, false, false, KS_MD_UNFUSED, false, false, KS_AUTO_NONE, false, false);
    f = all_fused(KS_GADGET_PRODUCT); f.ring_type = 1; f.dec_ok = f.md_ok = false;
    PIN("conjugate-invariant ring", f, KS_DIGITS_UNFUSED, false, false, KS_MD_UNFUSED, false, false, KS_AUTO_NONE, false, false);
    f = all_fused(KS_GADGET_PRODUCT); f.pw2 = true; f.keyd = false; f.levelP = 0; f.dec_ok = false;
    PIN("base-2 key with P", f, KS_DIGITS_WINDOWS, false, false, KS_MD_FUSED_ROWS, false, false, KS_AUTO_NONE, false, false);
    f.levelP = -1; f.md_ok = false;
    PIN("base-2 key without P", f, KS_DIGITS_WINDOWS, false, false, KS_MD_NONE, false, false, KS_AUTO_NONE, false, false);
    f = all_fused(KS_GADGET_PRODUCT); f.alias.out_is_addend = true;
    PIN("Relinearize in place", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_GADGET_PRODUCT); f.alias.crossed = true;
    PIN("Relinearize crossed", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_NONE, false, false);
    f = all_fused(KS_LAZY);
    PIN("lazy", f, KS_DIGITS_FUSED, true, false, KS_MD_NONE, false, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_HOISTED);
    PIN("hoisted", f, KS_DIGITS_GIVEN, false, false, KS_MD_FUSED_ROWS, false, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_AUTOMORPHISM);
    PIN("automorphism by epilogue scatter", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_EPILOGUE_SCATTER, false, true);
    f.alias.out_is_operand = f.alias.out_is_addend = true;
    PIN("automorphism in place: gathers over temporaries", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_GATHERS, false, false);
    f = all_fused(KS_AUTOMORPHISM); f.no_auto_scatter = true;
    PIN("automorphism, scatter switched off", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_GATHERS, false, true);
    f = all_fused(KS_AUTOMORPHISM_HOISTED);
    PIN("automorphism hoisted", f, KS_DIGITS_GIVEN, false, false, KS_MD_FUSED_ROWS, false, false, KS_AUTO_EPILOGUE_SCATTER, false, true);
    f = all_fused(KS_AUTOMORPHISM_HOISTED_LAZY);
    PIN("automorphism hoisted lazy by KsScatter", f, KS_DIGITS_GIVEN, false, false, KS_MD_NONE, false, false, KS_AUTO_KS_SCATTER, false, false);
    f.alias.crossed = true;
    PIN("automorphism hoisted lazy onto its input", f, KS_DIGITS_GIVEN, false, false, KS_MD_NONE, false, false, KS_AUTO_GATHERS, false, false);
    f = all_fused(KS_GIANT_STEP);
    PIN("giant step fused", f, KS_DIGITS_FUSED, true, false, KS_MD_NONE, false, false, KS_AUTO_KS_SCATTER, true, true);
    f.mac_giant_supported = false;
    PIN("giant step without the MAC giant tail", f, KS_DIGITS_FUSED, true, false, KS_MD_NONE, false, false, KS_AUTO_GATHERS, false, true);
    f = all_fused(KS_GIANT_STEP); f.no_giant_fusion = true;
    PIN("giant step, fusion switched off", f, KS_DIGITS_FUSED, true, false, KS_MD_NONE, false, false, KS_AUTO_GATHERS, false, true);
    f = all_fused(KS_MUL_RELIN);
    PIN("MulRelin: prologue, MAC and tensor epilogue", f, KS_DIGITS_FUSED, true, true, KS_MD_FUSED_MAC, false, true, KS_AUTO_NONE, false, true);
    f.alias.out_is_addend = true;
    PIN("MulRelin(res, res, res)", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_MAC, false, false, KS_AUTO_NONE, false, true);
    f = all_fused(KS_MUL_RELIN); f.no_prod_prologue = f.no_mac_epilogue = true;
    PIN("MulRelin, prologue and MAC epilogue switched off", f, KS_DIGITS_FUSED, true, false, KS_MD_FUSED_ROWS, true, true, KS_AUTO_NONE, false, true);
}

int main() {
    long combos = 0;
    for (int form = 0; form < KS_FORM_COUNT; form++)
        for (unsigned bits = 0; bits < 6 * (1u << 16); bits++) {
            unsigned b = bits & 0xffff;
            auto next = [&b]() { const bool v = b & 1; b >>= 1; return v; };
            KsFacts f;
            f.form = (KsForm)form;
            f.ring_type = next(); f.pw2 = next(); f.keyd = next(); f.levelP = next() ? 1 : -1; f.p_class2 = next(); f.f64_tables = next();
            f.dec_ok = next(); f.md_ok = next();
            // (the four *_supported predicates are one rule today, rows of 4096 or 8192: all off, each one alone off, all on)
            const int sup = (int)(bits >> 16);
            f.prod_in_supported = sup != 0 && sup != 1; f.scatter_supported = sup != 0 && sup != 2;
            f.mac_epilogue_supported = sup != 0 && sup != 3; f.mac_giant_supported = sup != 0 && sup != 4;
            f.alias.out_is_operand = next(); f.alias.out_is_addend = next(); f.alias.crossed = next();
            f.no_mac_epilogue = next(); f.no_prod_prologue = next(); f.no_tensor_epilogue = next(); f.no_auto_scatter = next();
            f.no_giant_fusion = next();
            // what the plans themselves guarantee (get_dec_plan / get_md_plan, api.cpp): a plan is ok on standard rings with
            // special primes only, and ks_call asks for no decomposition plan with a base-2 gadget
            if ((f.dec_ok || f.md_ok) && (f.ring_type != 0 || f.levelP < 0)) continue;
            if (f.dec_ok && f.pw2) continue;
            invariants(f);
            combos++;
        }
    pinned();
    std::printf("ks_route: %ld combinations, %ld checks, %ld failed\n", combos, g_checked, g_failed);
    if (g_failed) return 1;
    std::printf("PASS\n");
    return 0;
}
