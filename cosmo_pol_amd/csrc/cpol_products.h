// cpol_products.h -- which product a call carries behind its launch sequence, or why it is refused: A CALL CARRIES AT MOST ONE of
// superobservations, ensemble statistics (member_verify rides on them), spectrum moments, sweep histograms, gridded composites
// (fractions, with its objects, rides on them) and hydrometeor contributions.  Decided once per call by call_product() from the entry point and the pointers of
// cpol_outputs.  Plain C++ without HIP types, so that a host test can include it (tests/c_host/products_check.cpp,
// tests/test_call_product_cpu.py pin every pointer set at every entry point without a GPU).  run_sequence (cosmo_pol_hip.hip)
// gives the one product the one slot range of the call's array list and runs its *_plan and *_launch alone.
#pragma once

#include "../../include/cosmo_pol_amd.h"

enum { CALL_SWEEP = 0, CALL_MEMBERS, CALL_TIMED, CALL_COLUMNS };      // cpol_run_sweep, cpol_run_sweep_members (time_blend 0, 1), cpol_run_columns
enum { PRODUCT_NONE = 0, PRODUCT_SUPEROB, PRODUCT_MEMBER_STATS, PRODUCT_SPECTRUM_MOMENTS, PRODUCT_HISTOGRAM, PRODUCT_COMPOSITE, PRODUCT_SPECIES };

struct CallProduct {
    int product = PRODUCT_NONE;
    const char *refuse = nullptr;              // the call is refused before any product's own checks (the product is none then)
    bool at_entry = false;                     // ... by the entry point itself, ahead of its other argument checks
    const char *refuse_after_plan = nullptr;   // the call is refused once the product's *_plan has passed (the plan's refusals come first)
};

// A call with several faults reports the one it always reported: the order below is the rule.
inline CallProduct call_product(int entry, const cpol_outputs &o)
{
    const bool so = o.superob, ms = o.member_stats, mv = o.member_verify, sm = o.spectrum_moments, hg = o.histogram, cp = o.composite,
               fr = o.fractions, sp = o.species;
    CallProduct r;
    const auto refuse = [&](const char *why) { (r.product == PRODUCT_NONE ? r.refuse : r.refuse_after_plan) = why; return r; };
    if (entry == CALL_COLUMNS) {
        r.at_entry = so || cp || fr || hg || sm || ms || mv;
        if (so) return refuse("cpol_run_columns: superobservations (outputs->superob) are taken by cpol_run_sweep and cpol_run_sweep_members");
        if (cp) return refuse("cpol_run_columns: gridded composites (outputs->composite) are taken by cpol_run_sweep and cpol_run_sweep_members");
        if (fr) return refuse("cpol_run_columns: neighbourhood verification (outputs->fractions) is taken by cpol_run_sweep and cpol_run_sweep_members");
        if (hg) return refuse("cpol_run_columns: sweep histograms (outputs->histogram) are taken by cpol_run_sweep and cpol_run_sweep_members");
        if (sm) return refuse("cpol_run_columns: spectrum moments (outputs->spectrum_moments) are taken by cpol_run_sweep");
        if (ms) return refuse("cpol_run_columns: ensemble statistics (outputs->member_stats) are taken by cpol_run_sweep and cpol_run_sweep_members");
        if (mv) return refuse("cpol_run_columns: ensemble verification (outputs->member_verify) is taken by cpol_run_sweep and cpol_run_sweep_members");
        if (sp) {
            r.at_entry = true;
            return refuse("cpol_run_columns: hydrometeor contributions (outputs->species) are taken by cpol_run_sweep and a time-blended cpol_run_sweep_members");
        }
        return r;
    }
    if (sm && entry != CALL_SWEEP) {
        r.at_entry = true;
        return refuse("cpol_run_sweep_members: spectrum moments (outputs->spectrum_moments) are taken by cpol_run_sweep");
    }
    // (a composite and a histogram speak before the other product's own checks do)
    if (cp && (so || hg || ms || sm))
        return refuse("cpol_composite: not together with superobservations, histograms, ensemble statistics or spectrum moments in one call");
    if (hg && (so || ms || sm)) return refuse("cpol_histogram: not together with superobservations, ensemble statistics or spectrum moments in one call");
    // the first product present is the call's; whatever is present behind it refuses once that product's plan has passed
    if (so) r.product = PRODUCT_SUPEROB;
    if (mv && !ms) return refuse("cpol_member_verify: needs ensemble statistics (outputs->member_stats) in the same call");
    if (ms) {
        if (so) return refuse("cpol_member_stats: not together with superobservations (outputs->superob) in one call");
        if (entry == CALL_TIMED) return refuse("cpol_member_stats: a time-blended call (tables->time_blend) folds no members");
        r.product = PRODUCT_MEMBER_STATS;
    }
    if (sm) {
        if (so || ms) return refuse("cpol_spectrum_moments: not together with superobservations or ensemble statistics in one call");
        r.product = PRODUCT_SPECTRUM_MOMENTS;
    }
    if (hg) r.product = PRODUCT_HISTOGRAM;          // (alone but for a stray `fractions`: the refusals above)
    if (cp) r.product = PRODUCT_COMPOSITE;
    else if (fr) return refuse("cpol_fractions: needs a composite (outputs->composite) in the same call");
    // hydrometeor contributions: their refusals stand at the END of the order, so that a call with several faults reports what it
    // always reported; a pointer set without `species` decides exactly as before
    if (sp) {
        if (entry == CALL_MEMBERS)
            return refuse("cpol_run_sweep_members: hydrometeor contributions (outputs->species) are taken by cpol_run_sweep and by a time-blended call, not by the ensemble form");
        if (r.product != PRODUCT_NONE) return refuse("cpol_species: not together with another product in one call");
        r.product = PRODUCT_SPECIES;
    }
    return r;
}
