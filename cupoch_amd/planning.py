"""cupoch.planning mirror (src/cupoch/planning/planner.{h,cu}, python surface src/python/cupoch_pybind/planning):
Pos3DPlanner over a geometry.Graph roadmap.  The edges that collide with an obstacle (collision.compute_intersection of
the grid and the graph's lines at margin object_radius) are priced at +inf, then the shortest path is searched on the
GPU (mi_icp_graph_sssp).  Obstacles are VoxelGrid and OccupancyGrid; anything else is logged as unsupported.

The segment predicate is exactly symmetric in its end points (include/mi_icp.h, "segment-cell": mid is the same sum,
dst changes sign and only enters through |dst| and through products whose sign the absolute value drops), so both
directions of an undirected edge collide together and keep equal weights."""
import numpy as np

from . import collision, geometry

Path = list     # planning::Path: the points of a path (here a float32 [k, 3] numpy array is returned)


class PlannerBase:
    def __init__(self):
        self._obstacles = []

    def add_obstacle(self, obstacle):
        self._obstacles.append(obstacle)
        return self


class Pos3DPlanner(PlannerBase):
    def __init__(self, graph, object_radius=0.1, max_edge_distance=1.0):
        PlannerBase.__init__(self)
        self._graph = geometry.Graph(graph)
        self.object_radius = float(object_radius)
        self.max_edge_distance = float(max_edge_distance)

    def get_graph(self):
        return self._graph

    def update_graph(self):
        self._remove_collision_edges(self._graph)
        return self

    def _remove_collision_edges(self, graph):
        graph.set_edge_weights_from_distance()
        for obstacle in self._obstacles:
            if not isinstance(obstacle, (geometry.VoxelGrid, geometry.OccupancyGrid)):
                geometry._log_error("Unsupported obstacle type.")
                continue
            if len(graph.lines) == 0:
                continue
            res = collision.compute_intersection(obstacle, graph, self.object_radius, first_capacity=len(graph.lines))
            if res.is_collided():
                hit = graph.lines.tensor[res.collision_index_pairs[:, 1].long()]
                graph.set_edge_weights(hit, float("inf"))

    def find_path(self, start, goal):
        """-> the points of the shortest collision-free path from start to goal, float32 [k, 3] (start and goal
        included); empty when there is none.  A copy of the graph gets the start as node n (lazily) and the goal as
        node n + 1, each joined to every node nearer than max_edge_distance -- the goal also to the start."""
        g = geometry.Graph(self._graph)
        n = len(g.points)
        g.add_node_and_connect(start, self.max_edge_distance, True)
        g.add_node_and_connect(goal, self.max_edge_distance, False)
        if not g.is_constructed():          # (no edge reached either node)
            return np.zeros((0, 3), np.float32)
        self._remove_collision_edges(g)
        nodes, length = g.dijkstra_path(n, n + 1)
        if not nodes or not np.isfinite(length):
            return np.zeros((0, 3), np.float32)
        return g.points.tensor[nodes].cpu().numpy().astype(np.float32).reshape(-1, 3)
