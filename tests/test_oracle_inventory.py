"""Every oracle routine the GPU suite judges with is itself held to the reference.

tests/test_gpu_parity.py compares the kernels with oracle.<name>(...) bit for bit.  A judge that nothing holds to the reference could share a
kernel's bug and keep the suite green, so each name called there is either PINNED -- mapped to the CPU test that holds it to the reference
(tests/test_oracle_vs_reference.py) or to the reference's golden vectors (tests/test_oracle_golden.py) -- or one of a few HELPERS that judge
nothing on their own: samplers, key generators whose keys are judged by decryption, phases, distances and switches.  A new unpinned judge
fails here until it gets a pin.
"""
import ast
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))

PINNED = {
    "bk_to_dft": "test_oracle_vs_reference::test_blind_rotate_and_bootstrap_short_key",
    "ks_to_dft": "test_oracle_vs_reference::test_trlwe_keyswitch_automorphism_and_ga_bootstrap",
    "su_to_dft": "test_oracle_vs_reference::test_functional_bootstrap_unfolded",
    "torus_to_dft": "test_oracle_golden::test_fft_product_within_reference_tolerance",
    "dft_to_torus": "test_oracle_golden::test_fft_product_within_reference_tolerance",
    "poly_mul_fft": "test_oracle_vs_reference::test_fft_and_external_product_random",
    "poly_naive_mul": "test_oracle_vs_reference::test_fft_and_external_product_random",
    "poly_decompose_i": "test_oracle_vs_reference::test_integer_ops_random",
    "poly_permute": "test_oracle_vs_reference::test_integer_ops_random",
    "trlwe_extract_tlwe": "test_oracle_vs_reference::test_integer_ops_random",
    "trlwe_torus_packing": "test_oracle_vs_reference::test_by_component_product_order_is_held_to_the_reference_too",
    "trlwe_torus_packing_many_LUT": "test_oracle_vs_reference::test_fdfb_and_multivalue_short_key",
    "trlwe_mv_extract": "test_oracle_vs_reference::test_multivalue_phases",
    "external_product": "test_oracle_vs_reference::test_fft_and_external_product_random",
    "product_order": "test_oracle_vs_reference::test_by_component_product_order_is_held_to_the_reference_too",
    "blind_rotate": "test_oracle_vs_reference::test_blind_rotate_and_bootstrap_short_key",
    "blind_rotate_ga": "test_oracle_vs_reference::test_blind_rotate_ga_on_its_own",
    "pbs_preprocess": "test_oracle_vs_reference::test_programmable_bootstrap_preprocessing_range",
    "programmable_bootstrap": "test_oracle_vs_reference::test_programmable_bootstrap_preprocessing_range",
    "functional_bootstrap": "test_oracle_golden::test_bootstrap_phases_match_reference",
    "functional_bootstrap_wo_extract": "test_oracle_golden::test_bootstrap_phases_match_reference",
    "functional_bootstrap_ga": "test_oracle_vs_reference::test_trlwe_keyswitch_automorphism_and_ga_bootstrap",
    "functional_bootstrap_unfolded": "test_oracle_vs_reference::test_functional_bootstrap_unfolded",
    "functional_bootstrap_unfolded2_dft": "test_oracle_vs_reference::test_functional_bootstrap_unfolded",
    "multivalue_bootstrap_UBR_phase1": "test_oracle_vs_reference::test_functional_bootstrap_unfolded",
    "multivalue_bootstrap_UBR_phase2": "test_oracle_vs_reference::test_functional_bootstrap_unfolded",
    "multivalue_bootstrap_CLOT21": "test_oracle_vs_reference::test_fdfb_and_multivalue_short_key",
    "multivalue_bootstrap_phase1": "test_oracle_vs_reference::test_multivalue_phases",
    "multivalue_bootstrap_phase2": "test_oracle_vs_reference::test_multivalue_phases",
    "full_domain_functional_bootstrap": "test_oracle_vs_reference::test_fdfb_and_multivalue_short_key",
    "full_domain_functional_bootstrap_KS21": "test_oracle_vs_reference::test_public_mux_and_fdfb_KS21",
    "full_domain_functional_bootstrap_CLOT21": "test_oracle_vs_reference::test_tensor_product_tlwe_mul_and_fdfb_CLOT21",
    "functional_bootstrap_trgsw_phase1": "test_oracle_vs_reference::test_trgsw_accumulator_bootstrap",
    "functional_bootstrap_trgsw_phase2": "test_oracle_vs_reference::test_trgsw_accumulator_bootstrap",
    "circuit_bootstrap": "test_oracle_vs_reference::test_circuit_bootstrap_variants",
    "circuit_bootstrap_3": "test_oracle_vs_reference::test_circuit_bootstrap_variants",
    "public_mux": "test_oracle_vs_reference::test_public_mux_and_fdfb_KS21",
    "tlwe_keyswitch": "test_oracle_vs_reference::test_keyswitch_random",
    "trlwe_keyswitch": "test_oracle_vs_reference::test_trlwe_keyswitch_automorphism_and_ga_bootstrap",
    "trlwe_eval_automorphism": "test_oracle_vs_reference::test_trlwe_keyswitch_automorphism_and_ga_bootstrap",
    "trlwe_packing1_keyswitch": "test_oracle_vs_reference::test_reference_made_table_keys_and_their_key_switches",
    "trlwe_priv_keyswitch": "test_oracle_vs_reference::test_reference_made_table_keys_and_their_key_switches",
    "trlwe_priv_keyswitch_2": "test_oracle_vs_reference::test_circuit_bootstrap_pieces",
    "trlwe_lut_packing_keyswitch": "test_oracle_vs_reference::test_lut_packing_keyswitch_is_the_references",
    "gen_lut_packing_ks_key": "test_oracle_vs_reference::test_lut_packing_key_rows_decrypt_like_the_references",
    "trlwe_tensor_prod_fft": "test_oracle_vs_reference::test_tensor_product_tlwe_mul_and_fdfb_CLOT21",
    "tlwe_mul": "test_oracle_vs_reference::test_tensor_product_tlwe_mul_and_fdfb_CLOT21",
}

HELPERS = {
    # samplers and plain data
    "Rng", "u64", "double2torus", "gen_binary_key", "tlwe_sample", "trlwe_sample", "trgsw_monomial_sample",
    # key generators: their keys are judged by decryption (and the device's own generators are compared with them by phase)
    "gen_bootstrap_key", "gen_bootstrap_key_ga", "gen_bootstrap_key_unfolded", "gen_tlwe_ks_key", "gen_packing1_ks_key", "gen_priv_ks_key",
    "gen_priv_sk_ks_key", "gen_rl_key", "gen_automorphism_keyset",
    # phases, distances, the transform plan
    "tlwe_phase", "trlwe_phase", "torus_dist", "plan",
}


def _source(module):
    with open(os.path.join(HERE, module + ".py")) as fh:
        return fh.read()


def _judges():
    return set(re.findall(r"\boracle\.(\w+)\(", _source("test_gpu_parity")))


def _test_functions(module):
    src = _source(module)
    return {node.name: ast.get_source_segment(src, node) for node in ast.parse(src).body if isinstance(node, ast.FunctionDef) and node.name.startswith("test_")}


def test_every_gpu_judge_is_pinned_or_a_helper():
    judges = _judges()
    unpinned = sorted(judges - set(PINNED) - HELPERS)
    assert not unpinned, "oracle routines the GPU suite judges with but nothing holds to the reference: %s" % unpinned
    assert not set(PINNED) & HELPERS, sorted(set(PINNED) & HELPERS)
    stale = sorted((set(PINNED) | HELPERS) - judges)
    assert not stale, "listed here but no longer called by tests/test_gpu_parity.py: %s" % stale


def test_each_pin_calls_what_it_pins():
    """the pinning test exists and calls oracle.<name>( itself, so the map cannot point at a test that never looks at the routine"""
    tests = {}
    for name, test_id in sorted(PINNED.items()):
        module, func = test_id.split("::")
        if module not in tests:
            tests[module] = _test_functions(module)
        assert func in tests[module], "%s: no test %s" % (name, test_id)
        assert re.search(r"\boracle\.%s\(" % name, tests[module][func]), "%s does not call oracle.%s" % (test_id, name)
