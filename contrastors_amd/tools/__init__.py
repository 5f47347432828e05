"""Data-curation command-line tools built on contrastors_amd.search (consistency filtering, hard-negative mining)."""
