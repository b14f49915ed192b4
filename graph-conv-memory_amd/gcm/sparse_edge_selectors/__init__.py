"""Sparse edge selectors of the SparseGCM step (plugin API #3 of SURVEY 8b):
`forward(nodes, T, taus, B) -> torch.sparse_coo adjacency (batch, sink, source)`.

temporal.TemporalEdge   closed-form count + fill kernels
learned.LearnedEdge     closed-form causal candidates, pair gather, segmented gumbel softmax
spatial.SpatialKNNEdge  k nearest positions (radix selection per sink) as count + fill kernels
spatial.SpatialRadiusEdge  positions within a radius, causal or not, as count + fill kernels
"""
