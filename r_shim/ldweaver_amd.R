# Drop-in R definitions on top of the shim (same signatures as the reference).  NOT run in this repository
# (no R in the build image); the Python mirror ldweaver_amd/mi.py implements and tests the same logic.

.ldwamd_states_from_snpdat <- function(snp.dat) {
  # five L x N one-hot sparse matrices -> one raw L x N matrix, row-major, values 0..4
  st <- matrix(as.raw(0), nrow = snp.dat$nseq, ncol = snp.dat$nsnp)           # N x L column-major == L x N row-major
  for (k in 1:4) {
    m <- Matrix::t(snp.dat[[c("snp.matrix_C", "snp.matrix_G", "snp.matrix_T", "snp.matrix_N")[k]]])  # N x L
    idx <- Matrix::which(m)
    st[idx] <- as.raw(k)
  }
  st
}

# r05: options(ldwamd.devices = 0:7) -> one context per GPU of the node; the block loop (R/computePairwiseMI.R:103-116) and the
# sequence x sequence comparison of the Hamming weights are then shared over them INSIDE the library (ldw_mi_all_pairs_multi,
# ldw_hamming_weights_multi: worker threads, peer-to-peer gather into device ldwamd.devices[1]); results do not depend on it.
# options(ldwamd.sr_rows_stay = TRUE) (with several devices): the short-range rows — 99 % of the links — are NOT gathered; every device keeps
# the rows it computed, perform_MI_computation takes mergeNsort_sr_links_device below and the library runs the model's reductions over the
# devices (ldw_sr_len_quantiles_multi / _excess_stats_multi / _pvalues_multi); same sr_links.tsv.
.ldwamd_devices_set <- NULL
.ldwamd_use_devices <- function() {
  devs <- as.integer(getOption("ldwamd.devices", 0L))
  if (!identical(devs, .ldwamd_devices_set)) {
    .Call("ldwamd_set_devices", devs)
    .ldwamd_devices_set <<- devs
  }
  .Call("ldwamd_set_sr_rows_stay", isTRUE(getOption("ldwamd.sr_rows_stay", FALSE)) && length(devs) > 1)
  invisible(devs)
}

# r06: between jobs of a long session (or before another package allocates on the same GPUs): destroy the contexts and give the library's pooled device
# blocks and host buffers back; the next call makes its contexts again.  Returns the bytes released.
ldwamd_release <- function() {
  n <- .Call("ldwamd_release")
  .ldwamd_devices_set <<- NULL
  invisible(n)
}

.ACGTN2num <- function(nv, cv, ncores) invisible(.Call("ldwamd_ACGTN2num", nv, cv, as.integer(ncores)))

estimate_Hamming_distance_weights <- function(snp.dat, threshold = 0.1, mega_dset = F) {
  t0 <- Sys.time()
  .ldwamd_use_devices()
  .Call("ldwamd_set_alignment", .ldwamd_states_from_snpdat(snp.dat), snp.dat$nsnp, snp.dat$nseq)
  hdw <- .Call("ldwamd_hamming_weights", as.integer(snp.dat$nsnp * threshold), snp.dat$nseq)
  names(hdw) <- snp.dat$seq.names
  cat(paste("Done in", round(difftime(Sys.time(), t0, units = "secs"), 2), "s\n"))
  hdw
}

perform_MI_computation <- function(snp.dat, hdw, cds_var, ncores, lr_save_path = NULL, sr_save_path = NULL, plt_folder = NULL,
                                   sr_dist = 20000, lr_retain_links = 1e6, max_blk_sz = 10000, srp_cutoff = 3, runARACNE = TRUE,
                                   perform_SR_analysis_only = FALSE, order_links = T, mega_dset = F) {
  if (is.null(lr_save_path)) lr_save_path <- file.path(getwd(), "lr_links.tsv")
  if (is.null(sr_save_path)) sr_save_path <- file.path(getwd(), "sr_links.tsv")
  if (is.null(plt_folder)) plt_folder <- file.path(getwd(), "PLOTS")
  if (!file.exists(plt_folder)) dir.create(plt_folder)
  max_blk_sz <- round(max_blk_sz, -3)
  MI_cmp_blks <- make_blocks(snp.dat$nsnp, max_blk_sz)                       # reference's own helper, unchanged
  lr_links_approx <- 1
  if (!perform_SR_analysis_only) {                                           # R/computePairwiseMI.R:94-97, stays in R
    snp_subset <- min(snp.dat$nsnp, round(snp.dat$nsnp * 0.1))
    set.seed(1988)
    cnt <- sapply(snp.dat$POS[sample(snp.dat$nsnp, snp_subset)],
                  function(x) sum((0.5 * snp.dat$g - abs((x - snp.dat$POS) %% snp.dat$g - 0.5 * snp.dat$g)) > sr_dist))
    lr_links_approx <- sum(cnt) / snp_subset * snp.dat$nsnp / 2
  }
  .ldwamd_use_devices()
  .Call("ldwamd_set_alignment", .ldwamd_states_from_snpdat(snp.dat), snp.dat$nsnp, snp.dat$nseq)
  .Call("ldwamd_ctx_reserve", snp.dat$nsnp, snp.dat$nseq, max_blk_sz)        # r04: the pass's buffers, on a side thread, while the weights are set
  .Call("ldwamd_set_weights", as.numeric(hdw))
  .Call("ldwamd_set_snp_meta", as.numeric(snp.dat$r), as.raw(t(snp.dat$uqe)), as.integer(snp.dat$POS),
        as.integer(cds_var$paint), as.numeric(snp.dat$g))
  # r05: with options(ldwamd.native_tsv = TRUE) on ONE device lr_links.tsv is appended while the block loop runs, item by item — the reference's
  # per-block write.table(append = T) (:362): a job that dies leaves the finished blocks' rows
  stream_lr <- isTRUE(getOption("ldwamd.native_tsv", FALSE)) && !perform_SR_analysis_only && length(getOption("ldwamd.devices", 0L)) == 1
  if (stream_lr) .Call("ldwamd_lr_stream_begin", lr_save_path)
  res <- tryCatch(.Call("ldwamd_mi_all_pairs", as.integer(t(as.matrix(MI_cmp_blks))), sr_dist, lr_retain_links, lr_links_approx,
                        perform_SR_analysis_only, 0L),
                  error = function(e) { if (stream_lr) try(.Call("ldwamd_lr_stream_end"), silent = TRUE); stop(e) })
  if (stream_lr) .Call("ldwamd_lr_stream_end")
  to_df <- function(t) {
    # POS keeps its type (an INTEGER vector in the reference, src/getACGTNsites.cpp:97,173: pos1 / pos2 print as integers)
    pos2 <- snp.dat$POS[t[[1]] + 1]; pos1 <- snp.dat$POS[t[[2]] + 1]
    data.frame(pos1 = pos1, pos2 = pos2, clust1 = cds_var$paint[t[[2]] + 1], clust2 = cds_var$paint[t[[1]] + 1],
               len = 0.5 * snp.dat$g - abs((pos1 - pos2) %% snp.dat$g - 0.5 * snp.dat$g), MI = t[[3]])
  }
  # lr_links.tsv (:362): options(ldwamd.native_tsv = TRUE) writes it from the device table with the library's threaded writer
  # (same bytes as write.table, 1e6 rows in ~0.3 s instead of seconds); the default is R's own write.table
  native_lr <- FALSE
  if (!perform_SR_analysis_only && !stream_lr && length(res[[2]][[3]]) > 0) {
    if (isTRUE(getOption("ldwamd.native_tsv", FALSE))) {
      .Call("ldwamd_write_links_tsv_begin", 1L, lr_save_path)   # r04: written by host threads while mergeNsort_sr_links runs below
      native_lr <- TRUE
      on.exit(if (native_lr) try(.Call("ldwamd_write_links_tsv_end"), silent = TRUE), add = TRUE)   # (an error below must not leave the writer unjoined)
    } else write.table(to_df(res[[2]]), file = lr_save_path, append = T, quote = F, row.names = F, col.names = F, sep = "\t")
  }
  rows_stay <- isTRUE(getOption("ldwamd.sr_rows_stay", FALSE)) && length(getOption("ldwamd.devices", 0L)) > 1 && !perform_SR_analysis_only
  if (rows_stay) {   # r05: the table is spread over the devices and never comes into R: the model and ARACNE run where the rows lie
    sr_links_red <- mergeNsort_sr_links_device(snp.dat, cds_var, sr_dist, srp_cutoff, runARACNE, plt_folder)
    if (native_lr) { .Call("ldwamd_write_links_tsv_end"); native_lr <- FALSE }
    if (!runARACNE) warning("ARACNE not run, all values will be set to 1")
    if (order_links) { sr_links_red <- sr_links_red[order(sr_links_red$srp_max, decreasing = T), ]; rownames(sr_links_red) <- NULL }
    write.table(x = sr_links_red, file = sr_save_path, append = T, quote = F, row.names = F, col.names = F, sep = "\t")
    return(sr_links_red)
  }
  sr <- to_df(res[[1]])
  sr_links <- lapply(1:cds_var$nclust, function(i) sr[sr$clust1 == i | sr$clust2 == i, ])
  sr_links_all <- mergeNsort_sr_links(cds_var = cds_var, sr_links = sr_links, sr_dist = sr_dist, plt_path = plt_folder,
                                      srp_cutoff = srp_cutoff)                # reference's own function, unchanged
  sr_links_red <- sr_links_all$sr_links_red
  chk <- sr_links_all$sr_links_ARACNE_check
  if (native_lr) { .Call("ldwamd_write_links_tsv_end"); native_lr <- FALSE }                # lr_links.tsv is complete from here on
  if (runARACNE) {
    sr_links_red$ARACNE <- as.numeric(.Call("ldwamd_aracne", sr_links_red$pos1, sr_links_red$pos2, sr_links_red$MI,
                                            chk$pos1, chk$pos2, chk$MI))
  } else {
    warning("ARACNE not run, all values will be set to 1"); sr_links_red$ARACNE <- 1
  }
  if (order_links) { sr_links_red <- sr_links_red[order(sr_links_red$srp_max, decreasing = T), ]; rownames(sr_links_red) <- NULL }
  write.table(x = sr_links_red, file = sr_save_path, append = T, quote = F, row.names = F, col.names = F, sep = "\t")
  sr_links_red
}

# mergeNsort_sr_links + runARACNE with the short-range table left on the GPU by ldwamd_mi_all_pairs
# (R/computePairwiseMI.R:400-495): the O(#links) work runs in HBM, R keeps fastLm and fitdist.  Same rows, order and
# columns as the reference's sr_links_red; use it instead of the to_df(res[[1]]) / mergeNsort_sr_links lines of
# perform_MI_computation above when the table is too large to bring into R (config 5: 2.25e9 rows).
mergeNsort_sr_links_device <- function(snp.dat, cds_var, sr_dist, srp_cutoff, runARACNE = TRUE, plt_path = NULL) {
  nclust <- cds_var$nclust
  S <- ceiling(sr_dist) - 1
  q <- .Call("ldwamd_sr_len_quantiles", as.integer(nclust), sr_dist, 0.95)
  byrow <- function(v) matrix(v, ncol = S, byrow = TRUE)
  qlo <- byrow(q[[1]]); qhi <- byrow(q[[2]]); cnt <- byrow(q[[3]])
  md <- matrix(NA_real_, nrow = nclust, ncol = S)
  for (ci in 1:nclust) {
    has <- which(cnt[ci, ] > 0)
    index <- 1 + (cnt[ci, has] - 1) * 0.95; h <- index - floor(index)           # stats::quantile type 7
    mx <- ifelse(h > 0 & qhi[ci, has] != qlo[ci, has], (1 - h) * qlo[ci, has] + h * qhi[ci, has], qlo[ci, has])
    mod <- RcppArmadillo::fastLm(cbind(log(has), 1), log(mx))                    # :428
    md[ci, seq_along(has)] <- exp(fitted(mod))                                   # looked up by the VALUE of len (:448)
    if (!is.null(plt_path))                                                      # the maxvls table of the reference (:422-439)
      saveRDS(object = data.frame(len = has, max = mx, fit = md[ci, seq_along(has)]), file = file.path(plt_path, paste("c", ci, "_fit_data.rds", sep = "")))
  }
  st <- matrix(.Call("ldwamd_sr_excess_stats", as.integer(nclust), as.numeric(t(md))), ncol = 5, byrow = TRUE)
  shape <- t(sapply(1:nclust, function(ci) {
    n <- st[ci, 1]; slx <- st[ci, 4]; sl1x <- st[ci, 5]; m <- st[ci, 2] / n; v <- st[ci, 3] / n - m^2
    aux <- m * (1 - m) / v - 1                                                   # fitdistrplus' moment start
    nll <- function(p) if (any(p <= 0)) Inf else -((p[1] - 1) * slx + (p[2] - 1) * sl1x - n * lbeta(p[1], p[2]))
    p <- optim(c(m * aux, (1 - m) * aux), nll, control = list(reltol = 1e-14))$par   # the beta likelihood only needs these sums
    c(p, lbeta(p[1], p[2]))
  }))
  r <- .Call("ldwamd_sr_pvalues_aracne", as.integer(nclust), as.numeric(t(md)), as.numeric(t(shape)), srp_cutoff, runARACNE)
  pos2 <- snp.dat$POS[r[[2]] + 1]; pos1 <- snp.dat$POS[r[[3]] + 1]   # (integer like the reference's MI_df columns)
  df <- data.frame(clust_c = r[[5]], pos1 = pos1, pos2 = pos2, clust1 = cds_var$paint[r[[3]] + 1], clust2 = cds_var$paint[r[[2]] + 1],
                   len = 0.5 * snp.dat$g - abs((pos1 - pos2) %% snp.dat$g - 0.5 * snp.dat$g), MI = r[[4]], srp_max = r[[8]],
                   ARACNE = r[[9]])
  df[order(r[[7]], ifelse(r[[7]], r[[6]], r[[5]]), r[[1]]), ]                    # reference row order (:470-486)
}

# Numeric core of analyse_long_range_links (R/lr_analyser.R:72-118) on the tables the device holds after
# perform_MI_computation(): lr_links_red with its ARACNE column, in the reference's order.
# sr_links: the reduced short-range links, i.e. what sr_links.tsv holds / perform_MI_computation() returned (R/lr_analyser.R:67)
analyse_long_range_links_device <- function(snp.dat, cds_var, sr_links, are_lrlinks_ordered = F) {
  ia <- match(sr_links$pos2, snp.dat$POS); ib <- match(sr_links$pos1, snp.dat$POS)
  if (anyNA(ia) || anyNA(ib)) stop("sr_links holds positions that are not in snp.dat$POS")   # NA_integer_ must not reach the device as an index
  r <- .Call("ldwamd_lr_tukey_aracne", 5000, as.integer(ia - 1L), as.integer(ib - 1L), as.numeric(sr_links$MI))
  if (r[[8]]) warning("Not enough lr links pass the Tukey criteria, ~5000 top links were retained instead")
  pos2 <- snp.dat$POS[r[[2]] + 1]; pos1 <- snp.dat$POS[r[[3]] + 1]   # (integer like the reference's MI_df columns)
  df <- data.frame(pos1 = pos1, pos2 = pos2, clust1 = cds_var$paint[r[[3]] + 1], clust2 = cds_var$paint[r[[2]] + 1],
                   len = 0.5 * snp.dat$g - abs((pos1 - pos2) %% snp.dat$g - 0.5 * snp.dat$g), MI = r[[4]], ARACNE = r[[5]])
  if (!are_lrlinks_ordered) { df <- df[order(df$MI, decreasing = T), ]; rownames(df) <- NULL }
  list(lr_links_red = df, thresholds = r[[7]])
}

# The text of snpdat_to_fa (R/io_functions.R:363-417) from the resident alignment: snps_idx (1-based rows of snp.dat, output column
# order) as FASTA appended to aln_path, or as the tsv of write.table(fasta, sep = "\t", quote = F) (header = the positions, no leading field).
# Host memory stays O(chunk): no dense character matrix is built in R.
ldwamd_write_alignment <- function(snp.dat, aln_path, snps_idx, pos, format = "fasta") {
  if (format == "tsv") {
    writeLines(paste(as.integer(pos), collapse = "\t"), aln_path)
    .Call("ldwamd_write_alignment", aln_path, TRUE, 1L, as.integer(snps_idx - 1L), as.character(snp.dat$seq.names))
  } else {
    .Call("ldwamd_write_alignment", aln_path, TRUE, 0L, as.integer(snps_idx - 1L), as.character(snp.dat$seq.names))
  }
}

# The device halves of perform_snpEff_annotations (R/SnpEffAnnotations.R:29-103; rule table DESIGN.md 19).  ldwamd_annot_snps: one 12-word
# k_annot_snp record per SNP (columns) from the CDS segments (lo, hi, 1-based feature, each feature's segments in coding order) and the
# reference string.  ldwamd_annot_links: links_df ordered as add_annotations_to_links orders it, the annotation rows of both ends and the
# top hits of detect_top_hits (code per annotation row: "sy" "ns" "ig"; genreg: the cds strings, NA allowed).
ldwamd_annot_snps <- function(ref_string, seg_lo, seg_hi, seg_feature, strand, pos, alt_mask) {
  .Call("ldwamd_annot_snps", ref_string, as.integer(seg_lo), as.integer(seg_hi), as.integer(seg_feature - 1L), as.integer(strand),
        as.integer(pos), as.integer(alt_mask))
}
ldwamd_annot_links <- function(links_df, snp.dat, code, genreg, links_type = "SR", max_tophits = 250) {
  m <- .Call("ldwamd_annot_map", as.numeric(links_df$pos1), as.numeric(links_df$pos2), as.integer(snp.dat$POS))
  if (m[[2]] >= 0) stop(paste("a link position matches no SNP or several:", m[[2]] + 1))
  key <- if (links_type == "SR") links_df$srp_max else links_df$MI
  cds_id <- match(genreg, unique(genreg[!is.na(genreg)])) - 1L
  cds_id[is.na(cds_id)] <- -1L
  r <- .Call("ldwamd_annot_links", as.numeric(key), as.numeric(links_df$ARACNE), match(code, c("sy", "ns", "ig")) - 1L, as.integer(cds_id),
             as.numeric(max_tophits))
  list(snps = m[[1]] + 1L, order = r[[1]], row1 = r[[2]] + 1L, row2 = r[[3]] + 1L,
       links = c("syXsy", "syXns", "syXig", "nsXsy", "nsXns", "nsXig", "igXsy", "igXns", "igXig")[r[[4]] + 1L], top = r[[5]])
}

# Numeric core of genomewide_LDMap (R/LDSummaryPlot.R:55-109): the matrix heatmap3 is given.
genomewide_LDMap_device <- function(reducer = NULL, from = NULL, to = NULL) {
  .Call("ldwamd_ldmap", if (is.null(reducer)) 0L else as.integer(round(reducer)), if (is.null(from)) 0L else as.integer(round(from)),
        if (is.null(to)) 0L else as.integer(round(to)))
}

# estimate_variation_in_CDS (R/estimateCDSDiversity.R:27-123) with a gff3 annotation from parse_gff_file: masked SNP variation, per-CDS
# variation per base and the SNP paint on the device, the clustering at the exact k-means optimum (the reference's kmeans(nstart = 10) draws
# from an unseeded RNG).  quirk_mode = 0 reproduces painter's unrecorded single-SNP last run (that SNP may keep paint 0); 1 paints it from the
# left.  GenBank input and the cluster plot are not implemented.
ldwamd_estimate_variation_in_CDS <- function(snp.dat, ncores, gbk = NULL, gff = NULL, num_clusts_CDS = 3, clust_plt_path = NULL, mega_dset = FALSE,
                                             quirk_mode = 0L) {
  t0 <- Sys.time()
  if ((is.null(gbk) & is.null(gff)) | (!is.null(gbk) & !is.null(gff))) stop("Provide either one of gbk or gff")
  if (!is.null(gbk)) stop("ldweaver_amd: GenBank input is not implemented; use parse_gff_file")
  gff_cds <- gff$gff[tolower(gff$gff$type) == "cds", ]
  starts <- as.integer(gff_cds$start); ends <- as.integer(gff_cds$end)
  .ldwamd_use_devices()
  .Call("ldwamd_set_alignment", .ldwamd_states_from_snpdat(snp.dat), snp.dat$nsnp, snp.dat$nseq)
  v <- .Call("ldwamd_cds_variation", as.integer(snp.dat$POS), as.character(gff$ref), starts, ends)
  var_estimate <- v[[1]]; var_estimate[is.nan(var_estimate)] <- NA
  cds_idx <- !is.na(var_estimate)
  var_estimate <- var_estimate[cds_idx]; cds_start <- starts[cds_idx]; cds_end <- ends[cds_idx]
  km <- .Call("ldwamd_kmeans_1d", as.numeric(var_estimate), as.integer(num_clusts_CDS))
  clusts <- list(km_clst_ord = km[[1]], cutoff = km[[2]])
  p <- .Call("ldwamd_cds_paint", cds_start, cds_end, km[[1]], as.integer(num_clusts_CDS), as.integer(quirk_mode))
  paint <- p[[1]]
  if (p[[2]] > 0) warning(sprintf("SNP at POS %d keeps paint 0 (painter's unrecorded last run); quirk_mode = 1 paints it from the left",
                                  snp.dat$POS[which(paint == 0)[1]]))
  alpha <- c("A", "C", "G", "T", "*")
  alt <- vapply(v[[3]], function(m) paste(alpha[bitwAnd(m, c(1L, 2L, 4L, 8L, 16L)) > 0], collapse = ","), "")
  variation <- matrix(c(Matrix::rowSums(snp.dat$snp.matrix_A), Matrix::rowSums(snp.dat$snp.matrix_C), Matrix::rowSums(snp.dat$snp.matrix_G),
                        Matrix::rowSums(snp.dat$snp.matrix_T), Matrix::rowSums(snp.dat$snp.matrix_N)), ncol = snp.dat$nsnp, byrow = T)
  rownames(variation) <- c("A", "C", "G", "T", "N")
  cat(paste("Done in", round(difftime(Sys.time(), t0, units = "secs"), 2), "s\n"))
  list(var_estimate = var_estimate, cds_start = cds_start, cds_end = cds_end, clusts = clusts, paint = paint,
       ref = gff$ref[snp.dat$POS], alt = alt, allele_table = variation, nclust = num_clusts_CDS)
}
