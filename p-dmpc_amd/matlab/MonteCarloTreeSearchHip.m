classdef MonteCarloTreeSearchHip < OptimizerInterface
    % MONTECARLOTREESEARCHHIP  The sampled optimizer on an AMD MI355X through libpdmpc_hip.so.
    %
    % Drop-in replacement for MonteCarloTreeSearch (hlc/optimizer/graph_search/MonteCarloTreeSearch.m): same
    % run_optimizer signature, same random stream (mt19937ar seeded with time_step + vehicle_index, :32, generated
    % inside the library), same ControlResultsInfo fields.  Selected with options.optimizer_type =
    % OptimizerType.HipSampled (one more enum member and one more case in OptimizerInterface.get_optimizer,
    % see INTEGRATION.md).
    %
    % n_expansions_max is the reference's property (MonteCarloTreeSearch.m:8), read from config/mcts.json where that file exists
    % (:16-26) and handed to the library with pdmpc_mex('set_sampled_budget', ...): 250 runs the kernel the reference's default
    % always ran, any other value in 1 .. 16384 the kernel with a run-time budget (DESIGN.md section 3.18).
    %
    % n_members (no reference counterpart; config/mcts.json may set it too) is the seed ensemble of pdmpc_set_sampled_ensemble: every
    % vehicle of a step planned with pdmpc_mex('plan_step_sampled', ...) is planned by that many members on random streams of their own
    % -- member e draws from mt19937ar(seed + e * 1000003), member 0 is the reference's stream -- and gets the cheapest collision-free
    % plan, chosen on the device.  1 (the default) plans as the reference does (DESIGN.md section 3.18).
    %
    % Shipped as source like GraphSearchHip.m; the tested twin is pdmpc.optimizer.MonteCarloTreeSearchHip.

    properties (SetAccess = private)
        n_expansions_max (1, 1) double = 250; % MonteCarloTreeSearch.m:8
        n_members (1, 1) double = 1; % members per vehicle, 1 .. 16 (PDMPC_SAMPLED_ENSEMBLE_MAX)
    end

    properties (Access = private)
        handle uint64 = uint64(0);
        mpa_uploaded (1, 1) logical = false;
    end

    methods

        function obj = MonteCarloTreeSearchHip(options)
            obj = obj@OptimizerInterface();
            checker = double(options.are_any_obstacles_non_convex); % OptimizerInterface.m:36-46
            obj.handle = pdmpc_mex('create', options.Hp, checker, options.dt_seconds);

            % MonteCarloTreeSearch.m:16-26: config/mcts.json, kept out of version control, overrides the default
            file_path = fullfile('config', 'mcts.json'); % (relative to the working directory, as there)

            if isfile(file_path)
                mcts_config = jsondecode(fileread(file_path));

                if isfield(mcts_config, 'n_expansions_max')
                    obj.n_expansions_max = mcts_config.n_expansions_max;
                end

                if isfield(mcts_config, 'n_members')
                    obj.n_members = mcts_config.n_members;
                end

            end

            if obj.n_expansions_max ~= 250
                pdmpc_mex('set_sampled_budget', obj.handle, obj.n_expansions_max);
            end

            if obj.n_members ~= 1
                pdmpc_mex('set_sampled_ensemble', obj.handle, obj.n_members);
            end

        end

        function delete(obj)

            if obj.handle ~= 0
                pdmpc_mex('destroy', obj.handle);
            end

        end

        function info = run_optimizer(obj, vehicle_index, iter, mpa, options, time_step)
            assert(iter.amount == 1); % MonteCarloTreeSearch.m:50

            if ~obj.mpa_uploaded
                pdmpc_mex('upload_mpa', obj.handle, mpa.transition_matrix_single, mpa.maneuvers);
                obj.mpa_uploaded = true;
            end

            out = pdmpc_mex('plan_sampled', obj.handle, pdmpc_iter_struct(iter), time_step + vehicle_index);
            info = MonteCarloTreeSearchHip.info_from_record(options, out);
        end

    end

    methods (Static)

        function info = info_from_record(options, out)
            % ControlResultsInfo of a sampled record (one vehicle): what run_optimizer returns, and what
            % PrioritizedSequentialHipController's step (pdmpc_mex('plan_step_sampled', ...)) hands to finish_step_plan
            Hp = options.Hp;
            info = ControlResultsInfo(1, Hp);

            info.n_expanded = out.n_expanded; % MonteCarloTreeSearch.m:209
            info.is_exhausted = out.status ~= 0; % :212-215

            if info.is_exhausted
                return
            end

            % :217-248: the tree of the reference holds only the chosen descent's poses; rebuild that view
            tree = Tree();
            tree.x = out.path_nodes(:, 1)';
            tree.y = out.path_nodes(:, 2)';
            tree.yaw = out.path_nodes(:, 3)';
            tree.trim = out.path_nodes(:, 4)';
            tree.g = out.path_nodes(:, 5)';
            tree.h = out.path_nodes(:, 6)';
            tree.k = out.path_nodes(:, 7)';
            tree.parent = uint32(0:Hp);
            info.tree = tree;
            info.tree_path = 1:(Hp + 1);
            info.y_predicted = out.y_predicted(1:Hp, :)';
            info.shapes = arrayfun(@(k) squeeze(out.shapes(k, :, 1:out.shape_cols(k))), 1:Hp, UniformOutput = false);
            info.predicted_trims = out.predicted_trims(1:Hp);
            info.needs_fallback = false;
        end

    end

end
