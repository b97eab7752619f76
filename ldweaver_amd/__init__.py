"""MI355X-native LDWeaver: the entry points with the reference's names resolve lazily, so importing the package loads nothing."""

_EXPORTS = {
    "Engine": "engine", "kmeans_1d": "engine",
    "SnpDat": "snpdat", "CdsVar": "snpdat",
    "Annotation": "cds", "parse_gff_file": "cds", "estimate_variation_in_CDS": "cds",
    "GenBankRecord": "gbk", "parse_genbank_file": "gbk",
    "parse_fasta_alignment": "extract", "parse_fasta_SNP_alignment": "extract",
    "estimate_Hamming_distance_weights": "mi", "perform_MI_computation": "mi",
    "snpdat_to_fa": "output", "generate_Links_SNPS_fasta": "output", "write_output_for_gwes_explorer": "output",
    "read_TopHits": "output", "read_AnnotatedLinks": "output",
    "perform_snpEff_annotations": "annotate",
    "make_gwes_plots": "plots", "read_ShortRangeLinks": "plots", "read_LongRangeLinks": "plots",
    "read_links_native": "links_io",
    "create_tanglegram": "tanglegram",
    "LDWeaver": "driver", "cleanup": "driver",
    "view_tree": "tree", "read_newick": "tree", "midpoint_root": "tree", "ladderize": "tree",
    "nj_tree": "tree", "write_newick": "tree", "bootstrap_multiplicities": "tree",
    "snp_parsimony": "parsimony", "link_cochanges": "parsimony", "ancestral_states": "parsimony", "tip_sequences": "parsimony",
    "cochange_pvalue": "parsimony", "cochange_scan": "parsimony", "CochangeScan": "parsimony", "pick_min_co": "parsimony",
    "ld_decay": "decay", "LDDecay": "decay", "default_cuts": "decay",
    "snp_background": "background", "SnpBackground": "background", "link_apc": "background",
    "apc_links": "background", "pick_threshold": "background",
    "gene_map": "genemap", "GeneMap": "genemap", "segments_from_features": "genemap", "segments_from_annotation": "genemap", "segments_equal": "genemap",
    "sequence_clusters": "lineage", "link_lineage_mi": "lineage", "link_permutation_test": "lineage",
}
__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module(f".{_EXPORTS[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
