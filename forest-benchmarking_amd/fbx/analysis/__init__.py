"""Analysis helpers behind the reference's names (forest/benchmarking/analysis/)."""
