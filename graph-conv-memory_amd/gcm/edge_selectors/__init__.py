"""Dense edge selectors of the DenseGCM step (plugin API #1 of SURVEY 8b):
`forward(nodes, adj, weights, num_nodes, B) -> (adj, weights)`.

temporal.TemporalBackedge, dense.DenseEdge            index writes, folded into the step kernels
distance.EuclideanEdge / CosineEdge / SpatialEdge     fused pairwise distance + threshold kernels
knn.KNNEdge                                           k nearest stored nodes (L2 on pose slices / cosine):
                                                      distances, ranks and the adjacency row in one kernel
learned.LearnedEdge                                   candidate pairs + gumbel-softmax/STE kernels
                                                      around a user-replaceable edge network
typed.TypedEdge                                       several of the above side by side; which child selected an
                                                      entry goes into the `weights` plane as a bit code
                                                      (DenseGCM(edge_weights=True), gcm.nn.DenseRGCNConv)
"""
