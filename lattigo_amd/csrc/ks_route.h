// The launch route of a key switch, decided once: ks_route() is the only place where the facts a route depends on are combined.
// Host only, no HIP or library includes: tests/cpp/ks_route_test.cpp enumerates every combination of KsFacts on the CPU.
// DESIGN.md section 4 has the table of routes, section 9 the switches.
#pragma once

// the form of the call: he_gadget_product (he_relinearize, the key switches of he_apply_evaluation_key and ring packing), its lazy
// (also a leg of the RGSW generic route with several special primes) and hoisted forms, the three automorphisms, the giant step, MulRelin
enum KsForm { KS_GADGET_PRODUCT, KS_LAZY, KS_HOISTED, KS_AUTOMORPHISM, KS_AUTOMORPHISM_HOISTED, KS_AUTOMORPHISM_HOISTED_LAZY, KS_GIANT_STEP,
              KS_MUL_RELIN, KS_FORM_COUNT };
// aliasing within one entry: an output is the key switch's NTT-domain operand / the addend of its own component (MulRelin: any
// input) / the OTHER component's addend
struct KsAlias {
    bool out_is_operand = false, out_is_addend = false, crossed = false;
};
struct KsFacts {
    KsForm form = KS_GADGET_PRODUCT;
    int ring_type = 0, levelP = -1;  // 0 standard, 1 conjugate-invariant; the key's special primes, -1: none
    // the key is a base-2 gadget / has a double-precision copy; some P limb at this level / some modulus of the evaluator is below 2^47
    bool pw2 = false, keyd = false, p_class2 = false, f64_tables = false;
    // FusedPlan::ok of the decomposition plan and of the ModDown plan.  get_dec_plan / get_md_plan (api.cpp) say when a plan is
    // ok: standard rings with special primes only, and no decomposition plan is asked for with a base-2 gadget
    bool dec_ok = false, md_ok = false;
    // the *_supported(logN) predicates of kernels.hip
    bool prod_in_supported = false, scatter_supported = false, mac_epilogue_supported = false, mac_giant_supported = false;
    KsAlias alias;
    // the run-time switches
    bool no_mac_epilogue = false, no_prod_prologue = false, no_tensor_epilogue = false, no_auto_scatter = false, no_giant_fusion = false;
};
enum KsDigits { KS_DIGITS_WINDOWS, KS_DIGITS_FUSED, KS_DIGITS_UNFUSED, KS_DIGITS_GIVEN };
enum KsModDown { KS_MD_NONE, KS_MD_UNFUSED, KS_MD_FUSED_ROWS, KS_MD_FUSED_MAC };
enum KsAuto { KS_AUTO_NONE, KS_AUTO_EPILOGUE_SCATTER, KS_AUTO_KS_SCATTER, KS_AUTO_GATHERS };
// the answer; DESIGN.md section 4 says what each value launches
struct KsRoute {
    KsDigits digits = KS_DIGITS_UNFUSED;
    KsModDown moddown = KS_MD_NONE;
    KsAuto automorphism = KS_AUTO_NONE;
    bool mac_f64 = false, prod_prologue = false, acc_q_f64 = false, tensor_epilogue = false, giant_fused = false, tables_ok = false;
};
inline KsRoute ks_route(const KsFacts &f) {
    KsRoute r;
    const bool hasP = f.levelP >= 0, standard = f.ring_type == 0;
    const bool given = f.form == KS_HOISTED || f.form == KS_AUTOMORPHISM_HOISTED || f.form == KS_AUTOMORPHISM_HOISTED_LAZY;
    const bool lazy = f.form == KS_LAZY || f.form == KS_AUTOMORPHISM_HOISTED_LAZY || f.form == KS_GIANT_STEP;  // the accumulators are the result
    const bool automorphism = f.form == KS_AUTOMORPHISM || f.form == KS_AUTOMORPHISM_HOISTED;

    r.digits = given ? KS_DIGITS_GIVEN : f.pw2 ? KS_DIGITS_WINDOWS : f.dec_ok ? KS_DIGITS_FUSED : KS_DIGITS_UNFUSED;
    r.mac_f64 = r.digits == KS_DIGITS_FUSED && f.keyd;

    // an automorphism that writes onto its own inputs takes the gather form, which reads them all first: the epilogues would have
    // a thread read the addend at e and overwrite another position some other thread still has to read.  Standard ring only
    // (NthRoot = 2N).  HERING_NO_AUTO_SCATTER=1 keeps the gathers: the old sequence.
    const bool auto_alias = f.alias.out_is_operand || f.alias.out_is_addend || f.alias.crossed;
    if (automorphism)
        r.automorphism = (!f.no_auto_scatter && !auto_alias && f.md_ok && f.scatter_supported) ? KS_AUTO_EPILOGUE_SCATTER : KS_AUTO_GATHERS;
    if (f.form == KS_AUTOMORPHISM_HOISTED_LAZY) r.automorphism = (!f.no_auto_scatter && standard && !auto_alias) ? KS_AUTO_KS_SCATTER : KS_AUTO_GATHERS;
    // the giant step: with a double-precision key copy the NTT + MAC kernel needs its giant tail
    r.giant_fused = f.form == KS_GIANT_STEP && !f.no_auto_scatter && !f.no_giant_fusion && r.digits == KS_DIGITS_FUSED &&
                    (!f.keyd || f.mac_giant_supported);
    if (f.form == KS_GIANT_STEP) r.automorphism = r.giant_fused ? KS_AUTO_KS_SCATTER : KS_AUTO_GATHERS;

    if (!lazy && hasP) {
        r.moddown = f.md_ok ? KS_MD_FUSED_ROWS : KS_MD_UNFUSED;
        // ModDown inside the NTT + MAC kernel: possible when the P part does not depend on that kernel (no P limb of the
        // double-precision class) -- then the P accumulators come from ks_inner alone, are extended first, and the kernel over the
        // double-precision Q limbs forms the final outputs against its accumulators in registers.  The kernel writes the outputs
        // while other workgroups still read the operand -- the digits' own limbs: not when they alias (the gathers of an
        // automorphism read temporaries, which never do).
        const bool writes_operand = f.alias.out_is_operand && r.automorphism != KS_AUTO_GATHERS;
        if (f.md_ok && r.mac_f64 && !f.no_mac_epilogue && f.mac_epilogue_supported && !f.p_class2 && !writes_operand) r.moddown = KS_MD_FUSED_MAC;
    }
    // the fused rows epilogue can read double accumulators; the MAC epilogue keeps them in registers
    r.acc_q_f64 = r.moddown == KS_MD_FUSED_ROWS && r.mac_f64;
    // With a fused ModDown the tensor kernel forms c2 only: c0 / c1 are computed from the inputs where they are added.  Not when
    // an output aliases an input: the epilogue of one component would overwrite words the other still reads.
    r.tensor_epilogue = f.form == KS_MUL_RELIN && f.md_ok && !f.alias.out_is_addend && !f.no_tensor_epilogue;
    r.prod_prologue = r.tensor_epilogue && r.digits == KS_DIGITS_FUSED && f.f64_tables && f.prod_in_supported && !f.no_prod_prologue;

    // Entry tables: every launch that touches the callers' polynomials must be one of the table-capable ones (kernels.h,
    // View::tab).  The unfused and bit-window decompositions write the digits through pointers of their own.  Aliasing requests
    // never reach a table batch: their aliasing pattern is part of the batch key, and they are served one by one.
    switch (f.form) {
    case KS_LAZY: case KS_GIANT_STEP: r.tables_ok = r.digits == KS_DIGITS_FUSED; break;
    case KS_HOISTED: r.tables_ok = standard; break;
    // The key switches proper: the NTT-domain operand is read by the inverse row pass and as the digits' own limbs, the addends
    // and outputs by the epilogues (Automorphism: the final gathers) -- provided both fused plans exist.  An output equal to its
    // own component's addend is read and written by the same thread and batches normally
    case KS_GADGET_PRODUCT: r.tables_ok = f.dec_ok && f.md_ok && !f.alias.out_is_operand && !f.alias.crossed; break;
    case KS_AUTOMORPHISM: case KS_AUTOMORPHISM_HOISTED: r.tables_ok = f.dec_ok && f.md_ok && !auto_alias; break;
    // MulRelin: with a fused ModDown the inputs are read by the tensor kernel, the product prologue and the epilogues only
    case KS_MUL_RELIN: r.tables_ok = f.md_ok; break;
    default: break;  // (the hoisted lazy automorphism is served one by one)
    }
    return r;
}
