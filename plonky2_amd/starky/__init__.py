"""starky's lookup and cross-table-lookup stage on the GPU (include/p2hot.h, "starky" section)."""
