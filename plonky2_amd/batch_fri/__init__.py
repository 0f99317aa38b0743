"""Batch FRI -- mirror of plonky2/src/batch_fri/{oracle,prover}.rs: polynomials of several degrees in one BatchMerkleTree
(plonky2_amd.hash.batch_merkle_tree), opened by one FRI proof.  Poseidon configuration, one GPU, no blinding."""
from .oracle import BatchFriOracle, FriInstanceInfo  # noqa: F401
from .prover import batch_fri_committed_trees  # noqa: F401
