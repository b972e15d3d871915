// tests/probe/layers_run.cpp — Engine::exportLayers of the ROS adapter (csrc/ros_adapter/fpe_ros_adapter.hpp) RUN against the
// mock grid_map types of tests/probe/ros_mock and the real libfpe.so: a map file in (the format of adapter_run.cpp without the
// poses), the adapter's upload, one exportLayers call for all ten layers into buffers laid out like the map's own (column-major,
// its start index), and per layer a checksum of the buffer's 32-bit patterns out.  tests/test_gpu_layers_adapter.py builds this,
// runs it on the GPU box and compares with the same call through the Python binding.  Test infrastructure, not product.
#define FPE_WITH_ROS 1
#include "fpe_ros_adapter.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    // input: int32 rows, cols, start i, start j, roi[4]; f64 resolution, position x, y; then the two layers (rows * cols f32
    // each, column-major buffer with the start index applied)
    std::ifstream in(argv[1], std::ios::binary);
    int32_t hdr[8];
    double geo[3];
    in.read(reinterpret_cast<char*>(hdr), sizeof(hdr));
    in.read(reinterpret_cast<char*>(geo), sizeof(geo));
    grid_map::GridMap map;
    map.size = {{hdr[0], hdr[1]}};
    map.startIndex = {{hdr[2], hdr[3]}};
    map.resolution = geo[0];
    map.position = {{geo[1], geo[2]}};
    const size_t n = static_cast<size_t>(hdr[0]) * hdr[1];
    for (const char* name : {"traversability", "elevation"}) {
        grid_map::Matrix& m = map.layers[name];
        m.v.resize(n);
        in.read(reinterpret_cast<char*>(m.v.data()), static_cast<std::streamsize>(n * sizeof(float)));
    }
    if (!in) return 3;
    FILE* f = std::fopen(argv[2], "w");
    if (!f) return 4;
    try {
        fpe_ros::Engine eng(0);
        if (!eng.upload(map)) {
            std::fprintf(f, "upload failed: %s\n", eng.lastError());
            return 5;
        }
        fpe_params params;
        fpe_params_yaml(&params);
        // what a node does: one matrix per layer, sized like the map (here plain vectors: the mock's matrices are read-only)
        std::vector<std::vector<float>> store(FPE_LAYER_COUNT, std::vector<float>(n, -1.0f));
        std::vector<int32_t> ids;
        std::vector<float*> dst;
        for (int k = 0; k < FPE_LAYER_COUNT; ++k) {
            ids.push_back(FPE_LAYER_COUNT - 1 - k);  // (any order)
            dst.push_back(store[static_cast<size_t>(k)].data());
        }
        if (!eng.exportLayers(map, params, ids, dst, &hdr[4])) {
            std::fprintf(f, "exportLayers failed: %s\n", eng.lastError());
            return 7;
        }
        for (int k = 0; k < FPE_LAYER_COUNT; ++k) {
            // two position-dependent sums of the 32-bit patterns (mod 2^64)
            uint64_t s1 = 0, s2 = 0;
            for (size_t e = 0; e < n; ++e) {
                uint32_t u;
                std::memcpy(&u, &store[static_cast<size_t>(k)][e], 4);
                s1 += u;
                s2 += static_cast<uint64_t>(u) * (e + 1);
            }
            std::fprintf(f, "layer %d %llu %llu\n", ids[static_cast<size_t>(k)], static_cast<unsigned long long>(s1),
                         static_cast<unsigned long long>(s2));
        }
        // a map of another size is refused before the engine is asked (the destinations are sized by `like`)
        grid_map::GridMap other = map;
        other.size = {{hdr[0] + 1, hdr[1]}};
        std::fprintf(f, "mismatch %d\n", eng.exportLayers(other, params, ids, dst, nullptr) ? 1 : 0);
    } catch (const std::exception& e) {
        std::fprintf(f, "exception: %s\n", e.what());
        std::fclose(f);
        return 6;
    }
    std::fclose(f);
    return 0;
}
