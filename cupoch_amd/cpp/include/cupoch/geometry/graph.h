// cupoch/geometry/graph.h -- geometry::Graph<3> (reference: geometry/graph.h): a LineSet<3> whose lines are directed
// edges sorted by (first, second), with a CSR offset per node (edge_index_offsets_) and a weight per edge.  An
// undirected graph (is_directed_ == false, the default) holds both directions of every edge.  The sort, the lattice,
// the weight and removal updates and the shortest-path search run on the GPU through the mi_icp_graph_* family; the
// contract, the search's two predecessor tiers and its early end included, is in include/mi_icp.h ("graph").
// Not built: Graph<2>, CreateFromTriangleMesh, file I/O, visualisation.
#pragma once
#include <limits>
#include <memory>
#include <utility>

#include "cupoch/geometry/lineset.h"

namespace cupoch {
namespace geometry {

template <int Dim>
class Graph;

template <>
class Graph<3> : public LineSet<3> {
public:
    struct SSSPResult {
        SSSPResult(float shortest_distance = std::numeric_limits<float>::infinity(), int prev_index = -1)
            : shortest_distance_(shortest_distance), prev_index_(prev_index) {}
        float shortest_distance_;
        int prev_index_;
    };
    typedef utility::device_vector<SSSPResult> SSSPResultArray;
    typedef thrust::host_vector<SSSPResult> SSSPResultHostArray;

    Graph();
    Graph(const utility::device_vector<Eigen::Vector3f>& points);
    Graph(const thrust::host_vector<Eigen::Vector3f>& points);
    Graph(const Graph& other);
    ~Graph() override;

    thrust::host_vector<int> GetEdgeIndexOffsets() const { return edge_index_offsets_.to_host(); }
    void SetEdgeIndexOffsets(const thrust::host_vector<int>& edge_index_offsets) { edge_index_offsets_ = edge_index_offsets; }
    thrust::host_vector<float> GetEdgeWeights() const { return edge_weights_.to_host(); }
    void SetEdgeWeights(const thrust::host_vector<float>& edge_weights) { edge_weights_ = edge_weights; }

    bool HasWeights() const { return edge_weights_.size() > 0 && lines_.size() == edge_weights_.size(); }
    bool HasNodeColors() const { return node_colors_.size() > 0 && points_.size() == node_colors_.size(); }
    /// the lines are as ConstructGraph left them (an edge added lazily since then: not constructed)
    bool IsConstructed() const { return sorted_ && edge_index_offsets_.size() == points_.size() + 1 && lines_.size() == edge_weights_.size(); }

    Graph& Clear() override;

    Graph& ConstructGraph(bool set_edge_weights_from_distance = true);
    Graph& ConnectToNearestNeighbors(float max_edge_distance, size_t max_num_edges = 30);
    Graph& AddNodeAndConnect(const Eigen::Vector3f& point, float max_edge_distance = 0.0f, bool lazy_add = false);
    Graph& AddEdge(const Eigen::Vector2i& edge, float weight = 1.0, bool lazy_add = false);
    Graph& AddEdges(const utility::device_vector<Eigen::Vector2i>& edges,
                    const utility::device_vector<float>& weights = utility::device_vector<float>(), bool lazy_add = false);
    Graph& AddEdges(const thrust::host_vector<Eigen::Vector2i>& edges,
                    const thrust::host_vector<float>& weights = thrust::host_vector<float>(), bool lazy_add = false);
    Graph& RemoveEdge(const Eigen::Vector2i& edge);
    Graph& RemoveEdges(const utility::device_vector<Eigen::Vector2i>& edges);
    Graph& RemoveEdges(const thrust::host_vector<Eigen::Vector2i>& edges);
    Graph& PaintEdgeColor(const Eigen::Vector2i& edge, const Eigen::Vector3f& color);
    Graph& PaintEdgesColor(const thrust::host_vector<Eigen::Vector2i>& edges, const Eigen::Vector3f& color);
    Graph& PaintNodeColor(int node, const Eigen::Vector3f& color);
    /// paints the listed nodes (the reference paints all of them)
    Graph& PaintNodesColor(const thrust::host_vector<int>& nodes, const Eigen::Vector3f& color);
    Graph& SetEdgeWeightsFromDistance();
    Graph& SetEdgeWeights(const utility::device_vector<Eigen::Vector2i>& edges, float weight);

    std::shared_ptr<SSSPResultArray> DijkstraPaths(int start_node_index, int end_node_index = -1) const;
    std::shared_ptr<SSSPResultHostArray> DijkstraPathsHost(int start_node_index, int end_node_index = -1) const;
    /// (nodes from start to end, length); no path: (empty, +inf); start == end: ({start}, 0)
    std::pair<std::shared_ptr<thrust::host_vector<int>>, float> DijkstraPath(int start_node_index, int end_node_index) const;

    static std::shared_ptr<Graph<3>> CreateFromAxisAlignedBoundingBox(const AxisAlignedBoundingBox3& bbox, const Eigen::Vector3i& resolutions);
    static std::shared_ptr<Graph<3>> CreateFromAxisAlignedBoundingBox(const Eigen::Vector3f& min_bound, const Eigen::Vector3f& max_bound,
                                                                     const Eigen::Vector3i& resolutions);

public:
    utility::device_vector<int> edge_index_offsets_;
    utility::device_vector<float> edge_weights_;
    utility::device_vector<Eigen::Vector3f> node_colors_;
    bool is_directed_ = false;
    bool sorted_ = false;  // (not in the reference: see IsConstructed)
};

}  // namespace geometry
}  // namespace cupoch
